// Multi-view geometry on the tensors the model call already receives: the triangulation of the model's rays (the geometric
// baseline of a multi-view lifter) and the epipolar consistency score of the detections.
//
// Reference (MPL/lib/): multiviews/triangulate.py (the pymvg triangulation of the same detections), utils/calib.py:94-113
// distance_between_two_skew_lines, :116-169 smart_pseudo_remove_weight (every pair of views, per-view mean scaled by the view's
// confidence, weights above a threshold zeroed), which the multi-view datasets run in numpy per sample inside __getitem__.
// rays[v] (B,J,3) is a world point on the line of sight of view v (dataset/joints_dataset_mpl.py:872-904), centers[v] (B,1,3) the
// camera centre: line v goes through c_v along u_v = r_v - c_v.
//
// One work item = one (sample, joint).  The V tensors reach the kernels as pointer tables in the kernel arguments (as mpl_inputs
// does: no stacking copy).  Arithmetic is fp64 on the fp32 inputs -- a few hundred FLOPs per item against 24 V bytes read, and the
// normal equations of near-parallel rays at room-scale coordinates do not survive fp32 -- and rounded once into the fp32 outputs.
// No floating-point atomics and a fixed order of every sum: two runs give identical bits, and an item does not depend on its batch.
#include "common.hpp"

namespace mpl {

namespace {

constexpr int GEO_ITEMS = 64;      // items of one epipolar workgroup (their lines are staged in LDS once)
constexpr int GEO_SLICES = 4;      // waves of that workgroup: wave s scores views s, s + 4, ...

struct GeoViews {
    const float* rays[MPL_MAX_VIEWS];
    const float* centers[MPL_MAX_VIEWS];
    const float* conf[MPL_MAX_VIEWS];      // already at the confidence channel; all NULL = no confidences
    int conf_stride;
    int B, V, J;
};

__global__ __launch_bounds__(256) void triangulate_rays_kernel(const GeoViews p, float* __restrict__ points,
                                                               float* __restrict__ residual) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.B * p.J) return;
    const size_t b = (size_t)(idx / p.J);
    const double nan = __builtin_nan("");
    // origin shift: the mean of the sample's camera centres (room-scale coordinates stay out of the normal equations)
    double cm[3] = {0, 0, 0};
    for (int v = 0; v < p.V; ++v)
#pragma unroll
        for (int d = 0; d < 3; ++d) cm[d] += (double)p.centers[v][b * 3 + d];
#pragma unroll
    for (int d = 0; d < 3; ++d) cm[d] /= p.V;

    // A = sum w (I - d d^T) (symmetric: xx xy xz yy yz zz), bv = sum w (I - d d^T)(c - cm)
    double A[6] = {0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0}, W = 0;
    int n = 0;
    for (int v = 0; v < p.V; ++v) {
        double w = 1.0;
        if (p.conf[0]) w = (double)p.conf[v][(size_t)idx * p.conf_stride];
        if (!(w > 0.0) || !(w <= 1.79769313486231570e308)) continue;        // w <= 0, NaN or inf: the view does not take part
        double u[3], q[3], uu = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double c = (double)p.centers[v][b * 3 + d];
            u[d] = (double)p.rays[v][(size_t)idx * 3 + d] - c;
            q[d] = c - cm[d];
            uu += u[d] * u[d];
        }
        const double inv = 1.0 / sqrt(uu);
#pragma unroll
        for (int d = 0; d < 3; ++d) u[d] *= inv;
        const double uq = u[0] * q[0] + u[1] * q[1] + u[2] * q[2];
        A[0] += w * (1.0 - u[0] * u[0]);
        A[1] -= w * u[0] * u[1];
        A[2] -= w * u[0] * u[2];
        A[3] += w * (1.0 - u[1] * u[1]);
        A[4] -= w * u[1] * u[2];
        A[5] += w * (1.0 - u[2] * u[2]);
#pragma unroll
        for (int d = 0; d < 3; ++d) bv[d] += w * (q[d] - u[d] * uq);
        W += w;
        ++n;
    }
    float* po = points + (size_t)idx * 3;
    // adjugate of A / W; for two views its determinant is sin^2(angle) / 4
    const double iw = 1.0 / W;
    const double a = A[0] * iw, bb = A[1] * iw, c = A[2] * iw, d = A[3] * iw, e = A[4] * iw, f = A[5] * iw;
    const double c00 = d * f - e * e, c01 = c * e - bb * f, c02 = bb * e - c * d;
    const double det = a * c00 + bb * c01 + c * c02;
    if (n < 2 || det < 1e-10) {         // degenerate: fewer than two lines, or lines within ~2e-5 rad of parallel
        po[0] = po[1] = po[2] = (float)nan;
        residual[idx] = (float)nan;
        return;
    }
    const double c11 = a * f - c * c, c12 = bb * c - a * e, c22 = a * d - bb * bb;
    const double r0 = bv[0] * iw, r1 = bv[1] * iw, r2 = bv[2] * iw, id = 1.0 / det;
    double x[3];
    x[0] = cm[0] + (c00 * r0 + c01 * r1 + c02 * r2) * id;
    x[1] = cm[1] + (c01 * r0 + c11 * r1 + c12 * r2) * id;
    x[2] = cm[2] + (c02 * r0 + c12 * r1 + c22 * r2) * id;
#pragma unroll
    for (int k = 0; k < 3; ++k) po[k] = (float)x[k];

    // residual on the lines themselves (second read of the same 24 V bytes, from the cache).  The one-pass form
    // sum w q^T M q - y^T b cancels to nothing exactly where the residual matters, at lines that nearly meet.
    double s = 0;
    for (int v = 0; v < p.V; ++v) {
        double w = 1.0;
        if (p.conf[0]) w = (double)p.conf[v][(size_t)idx * p.conf_stride];
        if (!(w > 0.0) || !(w <= 1.79769313486231570e308)) continue;
        double u[3], t[3], uu = 0, ut = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double cc = (double)p.centers[v][b * 3 + k];
            u[k] = (double)p.rays[v][(size_t)idx * 3 + k] - cc;
            t[k] = x[k] - cc;
            uu += u[k] * u[k];
            ut += u[k] * t[k];
        }
        const double along = ut / uu;
        double perp2 = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double pk = t[k] - along * u[k];
            perp2 += pk * pk;
        }
        s += w * perp2;
    }
    residual[idx] = (float)sqrt(s * iw);
}

// LDS: [V][6][GEO_ITEMS] floats -- ray point then centre, the item index fastest (a wave reads 64 consecutive floats).
__global__ __launch_bounds__(GEO_ITEMS * GEO_SLICES) void epipolar_errors_kernel(const GeoViews p, float* __restrict__ err,
                                                                                 const float* __restrict__ weight_in,
                                                                                 float threshold, float* __restrict__ weight_out) {
    extern __shared__ float lines[];
    const int tid = threadIdx.x, V = p.V;
    const long long total = (long long)p.B * p.J, first = (long long)blockIdx.x * GEO_ITEMS;
    const int items = (int)(total - first < GEO_ITEMS ? total - first : GEO_ITEMS);
    for (int e = tid; e < V * GEO_ITEMS * 3; e += GEO_ITEMS * GEO_SLICES) {
        const int v = e / (GEO_ITEMS * 3), t = e % (GEO_ITEMS * 3), it = t / 3, d = t % 3;
        if (it < items) {
            const long long idx = first + it;
            lines[(v * 6 + d) * GEO_ITEMS + it] = p.rays[v][(size_t)idx * 3 + d];       // 192 consecutive floats per view
            lines[(v * 6 + 3 + d) * GEO_ITEMS + it] = p.centers[v][(size_t)(idx / p.J) * 3 + d];
        }
    }
    __syncthreads();
    const int it = tid % GEO_ITEMS, slice = tid / GEO_ITEMS;
    if (it >= items) return;
    const long long idx = first + it;
    const size_t b = (size_t)(idx / p.J), j = (size_t)(idx % p.J);
    for (int i = slice; i < V; i += GEO_SLICES) {        // wave-uniform
        double ui[3], ci[3], uui = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            ci[d] = (double)lines[(i * 6 + 3 + d) * GEO_ITEMS + it];
            ui[d] = (double)lines[(i * 6 + d) * GEO_ITEMS + it] - ci[d];
            uui += ui[d] * ui[d];
        }
        double sum = 0;
        for (int k = 0; k < V; ++k) {
            if (k == i) continue;
            double uk[3], dc[3], uuk = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double ck = (double)lines[(k * 6 + 3 + d) * GEO_ITEMS + it];
                uk[d] = (double)lines[(k * 6 + d) * GEO_ITEMS + it] - ck;
                dc[d] = ck - ci[d];
                uuk += uk[d] * uk[d];
            }
            // n = u_i x u_k; |(c_k - c_i) . n| / |n| does not depend on the lengths of u_i, u_k
            const double n0 = ui[1] * uk[2] - ui[2] * uk[1], n1 = ui[2] * uk[0] - ui[0] * uk[2], n2 = ui[0] * uk[1] - ui[1] * uk[0];
            const double nn = n0 * n0 + n1 * n1 + n2 * n2;
            if (nn < 1e-20 * uui * uuk) {
                // parallel lines (|d_i x d_k|^2 < 1e-20): the reference divides 0 by 0; the limit of its formula is the
                // distance of c_k to line i
                const double m0 = dc[1] * ui[2] - dc[2] * ui[1], m1 = dc[2] * ui[0] - dc[0] * ui[2], m2 = dc[0] * ui[1] - dc[1] * ui[0];
                sum += sqrt((m0 * m0 + m1 * m1 + m2 * m2) / uui);
            } else {
                sum += fabs(dc[0] * n0 + dc[1] * n1 + dc[2] * n2) / sqrt(nn);
            }
        }
        // calib.py:162-165: every pair counts, the confidence scales only the view's own total
        const double cf = p.conf[0] ? (double)p.conf[i][(size_t)idx * p.conf_stride] : 1.0;
        const double ev = cf * sum / (V - 1);
        const size_t at = (b * V + i) * p.J + j;
        err[at] = (float)ev;
        if (weight_out) weight_out[at] = ev > (double)threshold ? 0.f : weight_in[at];      // :167-168
    }
}

int geo_views(GeoViews& p, const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int B,
              int V, int J, int min_views) {
    if (!rays || !centers || B <= 0 || V <= 0 || J <= 0) return MPL_E_INVALID;
    if (V > MPL_MAX_VIEWS || J > 64 || V < min_views || (long long)B * J > (1ll << 30)) return MPL_E_UNSUPPORTED;
    if (conf && conf_stride != 1 && conf_stride != 3) return MPL_E_INVALID;
    for (int v = 0; v < MPL_MAX_VIEWS; ++v) {
        p.rays[v] = v < V ? rays[v] : nullptr;
        p.centers[v] = v < V ? centers[v] : nullptr;
        p.conf[v] = v < V && conf ? conf[v] : nullptr;
        if (v < V && (!p.rays[v] || !p.centers[v] || (conf && !p.conf[v]))) return MPL_E_INVALID;
        if (p.conf[v]) p.conf[v] += conf_stride - 1;       // (B,J,3) pose tensors: channel 2, read in place
    }
    p.conf_stride = conf ? conf_stride : 1;
    p.B = B; p.V = V; p.J = J;
    return MPL_OK;
}

}  // namespace

int launch_triangulate_rays(const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int B,
                            int V, int J, float* points, float* residual, hipStream_t s) {
    GeoViews p;
    if (int rc = geo_views(p, rays, centers, conf, conf_stride, B, V, J, 1)) return rc;
    if (!points || !residual) return MPL_E_INVALID;
    const long long total = (long long)B * J;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(triangulate_rays_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, points, residual);
    return hip_check_launch();
}

int launch_epipolar_errors(const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int B,
                           int V, int J, float* err, const float* weight_in, float threshold, float* weight_out, hipStream_t s) {
    GeoViews p;
    if (int rc = geo_views(p, rays, centers, conf, conf_stride, B, V, J, 2)) return rc;
    if (!err || (weight_in != nullptr) != (weight_out != nullptr)) return MPL_E_INVALID;
    const long long total = (long long)B * J;
    const size_t lds = (size_t)V * 6 * GEO_ITEMS * sizeof(float);        // 48 KiB at 32 views
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(epipolar_errors_kernel, dim3((unsigned)((total + GEO_ITEMS - 1) / GEO_ITEMS)), dim3(GEO_ITEMS * GEO_SLICES), lds,
                       s, p, err, weight_in, threshold, weight_out);
    return hip_check_launch();
}

}  // namespace mpl
