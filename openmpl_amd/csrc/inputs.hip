// Input preparation on the device: the step right before the path, which the reference runs
// in numpy per sample and per view inside DataLoader workers.
//
// Reference (MPL/lib/dataset/joints_dataset_mpl.py): normalize_screen_coordinates :817-820 -- (X/w)*2 - [1, h/w];
// camera normalisation :615-623; create_3d_ray_coords :872-904 -- world point at unit depth
// R^T [(x-cx)/fx, (y-cy)/fy, 1] + t; cam_center = t :646; model input = [x, y, conf] :772.
// From raw detections (B,V,J,2)+(B,V,J) and one calibration per view it writes exactly the V x (B,J,3) poses,
// V x (B,J,3) rays and V x (B,1,3) centers that mpl_forward consumes (150 B/pose of raw input instead of 1680 B).
// Arithmetic is fp64 and rounded once, like the reference's float64 numpy followed by .float().
#include "common.hpp"
#include "views.hpp"

namespace mpl {

struct PrepParams {                  // the pinhole launch: the kernel argument it has always had
    static constexpr bool DIST = false;
    ViewOutputs out;
    const float* px;
    const float* conf;
    const double* cams;   // device (V,16) camera records
    int B, V, J;
    double w, h;
    int norm_in, norm_cam;
};

struct PrepLensParams : PrepParams {
    static constexpr bool DIST = true;
    const double* dist;   // device (V,5) distortion records
};

// P::DIST: the ray goes through the undistorted pixel (views.hpp).  The lens comes with its own argument type, so that the pinhole
// instantiation is the kernel it was, argument layout included
template <class P>
__global__ __launch_bounds__(256) void prepare_inputs_kernel(const P p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int total = p.B * p.V * p.J;
    if (idx >= total) return;
    const int j = idx % p.J, v = (idx / p.J) % p.V, b = idx / (p.J * p.V);
    const size_t o = ((size_t)b * p.J + j) * 3;
    if constexpr (P::DIST)
        prepare_point_undistorted(p.cams + v * 16, distortion_of(p.dist, v), p.px[(size_t)idx * 2], p.px[(size_t)idx * 2 + 1],
                                  p.conf ? p.conf[idx] : 1.0f, p.w, p.h, p.norm_in, p.norm_cam, p.out.poses[v] + o, p.out.rays[v] + o,
                                  j == 0 ? p.out.centers[v] + (size_t)b * 3 : nullptr);
    else
        prepare_point(p.cams + v * 16, p.px[(size_t)idx * 2], p.px[(size_t)idx * 2 + 1], p.conf ? p.conf[idx] : 1.0f, p.w, p.h, p.norm_in,
                      p.norm_cam, p.out.poses[v] + o, p.out.rays[v] + o, j == 0 ? p.out.centers[v] + (size_t)b * 3 : nullptr);
}

int launch_prepare_inputs(const float* px, const float* conf, const double* cams_dev, const double* dist_dev, int B, int V, int J,
                          float w, float h, int norm_in, int norm_cam, float* const* poses, float* const* rays, float* const* centers,
                          hipStream_t s) {
    if (!px || !cams_dev || B <= 0 || V <= 0 || J <= 0 || w <= 0 || h <= 0) return MPL_E_INVALID;
    if ((long long)B * V * J > (1ll << 30)) return MPL_E_UNSUPPORTED;        // the item index is an int
    PrepLensParams p;
    if (const int rc = view_outputs_fill(p.out, poses, rays, centers, V)) return rc;
    p.px = px; p.conf = conf; p.cams = cams_dev; p.dist = dist_dev;
    p.B = B; p.V = V; p.J = J; p.w = w; p.h = h; p.norm_in = norm_in; p.norm_cam = norm_cam;
    const int total = B * V * J;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dist_dev)
        hipLaunchKernelGGL(prepare_inputs_kernel<PrepLensParams>, dim3((total + 255) / 256), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(prepare_inputs_kernel<PrepParams>, dim3((total + 255) / 256), dim3(256), 0, s, static_cast<const PrepParams&>(p));
    return hip_check_launch();
}

}  // namespace mpl
