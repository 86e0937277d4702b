// The data formats of the pose utilities, each stated once: the camera record with its distortion record (the lens model and its
// inverse), the model-input lists and the heatmap table.  inputs.hip, distortion.hip, heatmaps.hip, heatmap_render.hip, synth.hip and
// rpsm.hip read and write them through this header only.
#pragma once
#include "common.hpp"

namespace mpl {

// ---- the camera record: 16 doubles per view, fx fy cx cy | R row-major (world -> camera) | t (camera centre, world); pack_cameras
struct Camera {
    const double* c;
    __device__ __forceinline__ double fx() const { return c[0]; }
    __device__ __forceinline__ double fy() const { return c[1]; }
    __device__ __forceinline__ double cx() const { return c[2]; }
    __device__ __forceinline__ double cy() const { return c[3]; }
    __device__ __forceinline__ double r(int row, int col) const { return c[4 + 3 * row + col]; }
    __device__ __forceinline__ double t(int d) const { return c[13 + d]; }
};

constexpr double CAMERA_Z_MIN = 1e-9;        // a point at z_cam <= this is not in front of the camera

// x_cam = R (X - t)
__device__ __forceinline__ void camera_coords(const double* c, double X, double Y, double Z, double& xc, double& yc, double& zc) {
    const Camera cam{c};
    const double dx = X - cam.t(0), dy = Y - cam.t(1), dz = Z - cam.t(2);
    xc = cam.r(0, 0) * dx + cam.r(0, 1) * dy + cam.r(0, 2) * dz;
    yc = cam.r(1, 0) * dx + cam.r(1, 1) * dy + cam.r(1, 2) * dz;
    zc = cam.r(2, 0) * dx + cam.r(2, 1) * dy + cam.r(2, 2) * dz;
}

// ---- the distortion record: 5 doubles per view, k1 k2 k3 p1 p2; pack_distortion.  The lens model of the reference's
// project_point_radial (lib/multiviews/cameras.py:22-46, the H36M form), stated once with its inverse.
struct Distortion {
    double k1, k2, k3, p1, p2;
};

// view v of a (V,5) table; a null table is the pinhole: zeros, under which distort_normalized returns (y0, y1) bit for bit
__device__ __forceinline__ Distortion distortion_of(const double* dist, int v) {
    Distortion d{0.0, 0.0, 0.0, 0.0, 0.0};
    if (dist) {
        const double* q = dist + (size_t)v * 5;
        d.k1 = q[0]; d.k2 = q[1]; d.k3 = q[2]; d.p1 = q[3]; d.p2 = q[4];
    }
    return d;
}

// the five coefficients where a kernel has staged them; without LENS nothing is read and the pinhole folds at compile time
template <bool LENS>
__device__ __forceinline__ Distortion distortion_from(const double* five) {
    return Distortion{LENS ? five[0] : 0.0, LENS ? five[1] : 0.0, LENS ? five[2] : 0.0, LENS ? five[3] : 0.0, LENS ? five[4] : 0.0};
}

struct Normalized {                          // a point in normalised camera coordinates, x_cam.xy / z
    double x, y;
};

// The lens at one point with its analytic 2x2 Jacobian d y_d / d y: a pinhole point -> the same after the lens,
// y (1 + radial + tangential) + (p2, p1) r2.  The one statement of the polynomial; a caller that reads only part of the jet pays for
// that part.  Contraction is the compiler's default, as it was while rpsm_project held this expression; arguments and result go by
// value, which is what keeps rpsm's roundings in place
struct LensJet {
    double x, y;                             // y_d
    double j00, j01, j10, j11;
};

__device__ __forceinline__ LensJet distort_jet(double y0, double y1, Distortion d) {
    const double r2 = y0 * y0 + y1 * y1;
    const double g = 1.0 + (d.k1 * r2 + d.k2 * (r2 * r2) + d.k3 * (r2 * r2 * r2)) + (2.0 * d.p1 * y1 + 2.0 * d.p2 * y0);
    const double gr = d.k1 + 2.0 * d.k2 * r2 + 3.0 * d.k3 * (r2 * r2);                       // dg / dr2
    const double g0 = 2.0 * (gr * y0 + d.p2), g1 = 2.0 * (gr * y1 + d.p1);                   // dg / dy
    return LensJet{y0 * g + d.p2 * r2, y1 * g + d.p1 * r2,
                   g + y0 * g0 + 2.0 * d.p2 * y0, y0 * g1 + 2.0 * d.p2 * y1,
                   y1 * g0 + 2.0 * d.p1 * y0, g + y1 * g1 + 2.0 * d.p1 * y1};
}

__device__ __forceinline__ Normalized distort_normalized(double y0, double y1, Distortion d) {
    const LensJet jet = distort_jet(y0, y1, d);
    return Normalized{jet.x, jet.y};
}

// a point after the lens -> its pixel, f y_d + c
struct Pixel {
    double x, y;
};

__device__ __forceinline__ Pixel pixel_of(const Camera& cam, double yd0, double yd1) {
    return Pixel{cam.fx() * yd0 + cam.cx(), cam.fy() * yd1 + cam.cy()};
}

constexpr int UNDISTORT_MAX_ITER = 20;       // a guard: the coefficient sets of the tests take at most 4 on a centred subject
constexpr double UNDISTORT_TOL = 1e-14;

// The inverse: Newton from y = y_d with the analytic Jacobian.  false (not invertible): an iterate with det J <= 0 -- the point lies
// beyond the fold of the polynomial --, a non-finite value, or no step below UNDISTORT_TOL * max(1, |y|_inf) within the cap; y0, y1
// then hold the last iterate.  With zero coefficients the first residual is exactly 0 and y = y_d bit for bit.
__device__ __forceinline__ bool undistort_normalized(double yd0, double yd1, Distortion d, double& y0, double& y1) {
    y0 = yd0;
    y1 = yd1;
    for (int it = 0; it < UNDISTORT_MAX_ITER; ++it) {
        const LensJet jet = distort_jet(y0, y1, d);
        const double det = jet.j00 * jet.j11 - jet.j01 * jet.j10;
        if (!(det > 0.0)) return false;
        const double f0 = jet.x - yd0, f1 = jet.y - yd1;
        const double s0 = (jet.j11 * f0 - jet.j01 * f1) / det, s1 = (jet.j00 * f1 - jet.j10 * f0) / det;
        y0 -= s0;
        y1 -= s1;
        if (!(isfinite(y0) && isfinite(y1))) return false;
        if (fmax(fabs(s0), fabs(s1)) <= UNDISTORT_TOL * fmax(1.0, fmax(fabs(y0), fabs(y1)))) return true;
    }
    return false;
}

// The observed pixel (x, y) of view c -> the pixel a pinhole camera would have seen, (x + fx D0, y + fy D1) with D = y_u - y_d in
// normalised coordinates: zero coefficients give D = 0 and the input.  false: not invertible, (xu, yu) is then not to be used.
__device__ __forceinline__ bool undistort_pixel(const double* c, Distortion d, double x, double y, double& xu, double& yu) {
    const Camera cam{c};
    const double yd0 = (x - cam.cx()) / cam.fx(), yd1 = (y - cam.cy()) / cam.fy();
    double y0, y1;
    const bool ok = undistort_normalized(yd0, yd1, d, y0, y1);
    xu = x + cam.fx() * (y0 - yd0);
    yu = y + cam.fy() * (y1 - yd1);
    return ok;
}

// The arithmetic of input preparation for one (sample, view, joint).  Reference: inputs.hip.
// c: the view's record; (x, y) the pixel; po / ro the item's 3 floats in poses[v] / rays[v]; co the sample's 3 floats in centers[v],
// or null in every thread but the one of joint 0.  fp64, every output rounded once.
__device__ __forceinline__ void prepare_point(const double* c, double x, double y, float cf, double w, double h, int norm_in,
                                              int norm_cam, float* po, float* ro, float* co) {
    const Camera cam{c};
    double fx = cam.fx(), fy = cam.fy(), cx = cam.cx(), cy = cam.cy();
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
    for (int d = 0; d < 3; ++d) ro[d] = (float)(u0 * cam.r(0, d) + u1 * cam.r(1, d) + u2 * cam.r(2, d) + cam.t(d));   // R^T u + t
    if (co) {
#pragma unroll
        for (int d = 0; d < 3; ++d) co[d] = (float)cam.t(d);
    }
}

// The same under a lens: the ray is that of prepare_point on the undistorted pixel, whose poses are dropped; poses hold the observed
// pixel, normalised as prepare_point does, and the confidence.  A pixel that is not invertible keeps its pinhole ray and gets
// confidence 0, like a missing joint: every geometric consumer then drops the view.  prepare_point itself stays as it is, so that
// the pinhole kernels (decode_kernel among them) keep their code.
__device__ __forceinline__ void prepare_point_undistorted(const double* c, Distortion d, double x, double y, float cf, double w,
                                                          double h, int norm_in, int norm_cam, float* po, float* ro, float* co) {
    double xu, yu;
    if (!undistort_pixel(c, d, x, y, xu, yu)) {
        xu = x;
        yu = y;
        cf = 0.0f;
    }
    float dropped[3];
    prepare_point(c, xu, yu, cf, w, h, norm_in, norm_cam, dropped, ro, co);
    if (norm_in) {
        x = (x / w) * 2.0 - 1.0;
        y = (y / w) * 2.0 - h / w;
    }
    po[0] = (float)x;
    po[1] = (float)y;
    po[2] = cf;
}

// ---- the model-input lists: poses, rays, centers, V tensors (B,J,3), (B,J,3), (B,1,3) each; what mpl_forward consumes
struct ViewOutputs {
    float* poses[MPL_MAX_VIEWS];
    float* rays[MPL_MAX_VIEWS];
    float* centers[MPL_MAX_VIEWS];
};

// The caller's three tables of V device pointers -> o: entries below V copied and required, the rest nulled.  present = false: the
// lists are absent as a group, nothing is read and every entry is nulled.
inline int view_outputs_fill(ViewOutputs& o, float* const* poses, float* const* rays, float* const* centers, int V, bool present = true) {
    if (V > MPL_MAX_VIEWS || (present && (!poses || !rays || !centers))) return MPL_E_INVALID;
    for (int v = 0; v < MPL_MAX_VIEWS; ++v) {
        const bool on = present && v < V;
        o.poses[v] = on ? poses[v] : nullptr;
        o.rays[v] = on ? rays[v] : nullptr;
        o.centers[v] = on ? centers[v] : nullptr;
        if (on && (!o.poses[v] || !o.rays[v] || !o.centers[v])) return MPL_E_INVALID;
    }
    return MPL_OK;
}

// ---- the heatmap table: view v is (B,J,H,W) values of `dtype` (MPL_HM_*) at hm[v], its (J,H,W) block dense, sample b at element
// b * batch_stride -- V separate tensors and one (B,V,J,H,W) tensor are both read where they lie
template <int DT>
__device__ __forceinline__ float hm_widen16(unsigned u) {
    if (DT == MPL_HM_BF16) return __uint_as_float(u << 16);
    return (float)__builtin_bit_cast(_Float16, (unsigned short)u);
}

// element i of a map of dtype dt, widened exactly
__device__ __forceinline__ float hm_fetch(const void* base, size_t i, int dt) {
    if (dt == MPL_HM_F32) return static_cast<const float*>(base)[i];
    const unsigned u = static_cast<const unsigned short*>(base)[i];
    return dt == MPL_HM_BF16 ? hm_widen16<MPL_HM_BF16>(u) : hm_widen16<MPL_HM_F16>(u);
}

// The way back, for the kernel that writes maps: an fp64 value rounded ONCE (to nearest, ties to even) to dtype DT, denormals
// kept.  fp32 is the hardware conversion.  A 16-bit type goes through an fp32 that is rounded to odd -- truncated towards zero with
// the last bit set when anything was lost -- which has 13 (fp16) or 16 (bf16) bits more than the target, so the second rounding
// sees on which side of every tie the fp64 value lay.
template <int DT>
__device__ __forceinline__ unsigned hm_narrow(double x) {
    float f = (float)x;
    if (DT == MPL_HM_F32) return __float_as_uint(f);
    unsigned u = __float_as_uint(f);
    if ((double)f != x && x == x && (u & 0x7f800000u) != 0x7f800000u) {      // inexact, and neither NaN nor overflowed
        if (fabs((double)f) > fabs(x)) u -= 1;                               // the magnitude below: towards zero
        u |= 1;
        f = __uint_as_float(u);
    }
    if (DT == MPL_HM_F16) return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f);
    if (f != f) return 0x7fc0u | (u >> 31 << 15);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

struct HeatmapTable {
    const void* hm[MPL_MAX_VIEWS];
    long long batch_stride;                  // elements
    int dtype, B, V, J, H, W;

    // the (H,W) map of joint j of sample b in view v; es: the element size, a constant in a kernel compiled for one dtype.
    // H * W is at most 2^20 (heatmap_table_fill), so the product is taken in int
    __device__ __forceinline__ const void* map(int b, int v, int j, size_t es) const {
        return static_cast<const char*>(hm[v]) + ((size_t)b * (size_t)batch_stride + (size_t)j * (size_t)(H * W)) * es;
    }
    __device__ __forceinline__ const void* map(int b, int v, int j) const { return map(b, v, j, dtype == MPL_HM_F32 ? 4 : 2); }
};

// The caller's table of V device pointers and its sizes (all positive) -> t.  MPL_E_INVALID: no table, an unknown dtype, a batch
// stride below J*H*W, a null entry below V; MPL_E_UNSUPPORTED: V > MPL_MAX_VIEWS, H*W > 2^20.
inline int heatmap_table_fill(HeatmapTable& t, const void* const* heatmaps, int dtype, long long batch_stride, int B, int V, int J, int H,
                              int W) {
    if (!heatmaps || (dtype != MPL_HM_F32 && dtype != MPL_HM_F16 && dtype != MPL_HM_BF16)) return MPL_E_INVALID;
    if (V > MPL_MAX_VIEWS || (long long)H * W > (1ll << 20)) return MPL_E_UNSUPPORTED;
    if (batch_stride < (long long)J * H * W) return MPL_E_INVALID;
    for (int v = 0; v < MPL_MAX_VIEWS; ++v) {
        t.hm[v] = v < V ? heatmaps[v] : nullptr;
        if (v < V && !t.hm[v]) return MPL_E_INVALID;
    }
    t.batch_stride = batch_stride; t.dtype = dtype; t.B = B; t.V = V; t.J = J; t.H = H; t.W = W;
    return MPL_OK;
}

}  // namespace mpl
