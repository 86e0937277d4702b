// Pixels through the lens and back on the device: the radial / tangential polynomial of the reference's project_point_radial
// (MPL/lib/multiviews/cameras.py:22-46) and its Newton inverse, both stated in views.hpp.  The reference undistorts on the host,
// inside pymvg (lib/multiviews/triangulate.py:26-38).
//
// One work item per (sample, view, joint), one launch, no LDS, no atomics; fp64 on the fp32 pixel, every output rounded once.  Both
// directions write the input plus a correction formed in normalised coordinates, so zero coefficients return the input.
#include "common.hpp"
#include "views.hpp"

namespace mpl {

struct UndistortParams {
    const float* px;          // (B,V,J,2)
    const double* cams;       // device (V,16) camera records
    const double* dist;       // device (V,5) distortion records
    float* out;               // (B,V,J,2)
    unsigned char* valid;     // (B,V,J) or null
    int total, V, J;
};

template <int DIRECTION>
__global__ __launch_bounds__(256) void undistort_points_kernel(const UndistortParams p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int v = (idx / p.J) % p.V;
    const double* c = p.cams + v * 16;
    const Distortion d = distortion_of(p.dist, v);
    const double x = p.px[(size_t)idx * 2], y = p.px[(size_t)idx * 2 + 1];
    double xo, yo;
    bool ok = true;
    if (DIRECTION == MPL_DISTORT_REMOVE) {
        ok = undistort_pixel(c, d, x, y, xo, yo);
        if (!ok) xo = yo = __builtin_nan("");
    } else {
        const Camera cam{c};
        const double y0 = (x - cam.cx()) / cam.fx(), y1 = (y - cam.cy()) / cam.fy();
        const Normalized yd = distort_normalized(y0, y1, d);
        xo = x + cam.fx() * (yd.x - y0);
        yo = y + cam.fy() * (yd.y - y1);
    }
    p.out[(size_t)idx * 2] = (float)xo;
    p.out[(size_t)idx * 2 + 1] = (float)yo;
    if (p.valid) p.valid[idx] = ok ? 1 : 0;
}

int launch_undistort_points(const float* px, const double* cams_dev, const double* dist_dev, int B, int V, int J, int direction,
                            float* out_px, unsigned char* out_valid, hipStream_t s) {
    if (!px || !cams_dev || !dist_dev || !out_px || B <= 0 || V <= 0 || V > MPL_MAX_VIEWS || J <= 0) return MPL_E_INVALID;
    if (direction != MPL_DISTORT_REMOVE && direction != MPL_DISTORT_APPLY) return MPL_E_INVALID;
    if ((long long)B * V * J > (1ll << 30)) return MPL_E_UNSUPPORTED;
    UndistortParams p;
    p.px = px; p.cams = cams_dev; p.dist = dist_dev; p.out = out_px; p.valid = out_valid;
    p.total = B * V * J; p.V = V; p.J = J;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (direction == MPL_DISTORT_REMOVE)
        hipLaunchKernelGGL(undistort_points_kernel<MPL_DISTORT_REMOVE>, dim3((p.total + 255) / 256), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(undistort_points_kernel<MPL_DISTORT_APPLY>, dim3((p.total + 255) / 256), dim3(256), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
