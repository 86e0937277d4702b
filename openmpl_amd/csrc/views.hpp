// The three data formats of the pose utilities, each stated once: the camera record, the model-input lists and the heatmap table.
// inputs.hip, heatmaps.hip, heatmap_render.hip, synth.hip and rpsm.hip read and write them through this header only (DESIGN.md
// section 7).
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
