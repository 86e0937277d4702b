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
// triangulate_robust_kernel adds what a deployed baseline has: the reference's per-joint view selection by confidence
// (multiviews/triangulate.py:88-112) and an exhaustive pair consensus, then the same least-squares fit on the inliers.
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

constexpr double DET_MIN = 1e-10;         // det(A / sum w) below this: degenerate (two views: sin^2(angle) / 4)

// The lines of one item as the kernels hold them: in the V tensors themselves, or staged in LDS (item index fastest).
struct GlobalLines {
    const GeoViews& p;
    size_t b, idx;
    __device__ double ray(int v, int d) const { return (double)p.rays[v][idx * 3 + d]; }
    __device__ double center(int v, int d) const { return (double)p.centers[v][b * 3 + d]; }
    __device__ double weight(int v) const { return p.conf[0] ? (double)p.conf[v][idx * p.conf_stride] : 1.0; }
};

struct StagedLines {
    const float* lines;     // [V][6][GEO_ITEMS]: ray point, then centre
    const float* conf;      // [V][GEO_ITEMS] or NULL
    int it;
    __device__ double ray(int v, int d) const { return (double)lines[(v * 6 + d) * GEO_ITEMS + it]; }
    __device__ double center(int v, int d) const { return (double)lines[(v * 6 + 3 + d) * GEO_ITEMS + it]; }
    __device__ double weight(int v) const { return conf ? (double)conf[v * GEO_ITEMS + it] : 1.0; }
};

// A = sum w (I - d d^T) (symmetric: xx xy xz yy yz zz), bv = sum w (I - d d^T)(c - cm), W = sum w
struct Normal {
    double A[6] = {0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0}, W = 0;
};

template <class Lines>
__device__ inline void normal_add(Normal& s, const Lines& ln, int v, double w, const double cm[3]) {
    double u[3], q[3], uu = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double c = ln.center(v, d);
        u[d] = ln.ray(v, d) - c;
        q[d] = c - cm[d];
        uu += u[d] * u[d];
    }
    const double inv = 1.0 / sqrt(uu);
#pragma unroll
    for (int d = 0; d < 3; ++d) u[d] *= inv;
    const double uq = u[0] * q[0] + u[1] * q[1] + u[2] * q[2];
    s.A[0] += w * (1.0 - u[0] * u[0]);
    s.A[1] -= w * u[0] * u[1];
    s.A[2] -= w * u[0] * u[2];
    s.A[3] += w * (1.0 - u[1] * u[1]);
    s.A[4] -= w * u[1] * u[2];
    s.A[5] += w * (1.0 - u[2] * u[2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) s.bv[d] += w * (q[d] - u[d] * uq);
    s.W += w;
}

// x = cm + A^-1 bv by the adjugate of A / W (for two views its determinant is sin^2(angle) / 4); false where it is below DET_MIN:
// lines within ~2e-5 rad of parallel
__device__ inline bool normal_solve(const Normal& s, const double cm[3], double x[3]) {
    const double iw = 1.0 / s.W;
    const double a = s.A[0] * iw, bb = s.A[1] * iw, c = s.A[2] * iw, d = s.A[3] * iw, e = s.A[4] * iw, f = s.A[5] * iw;
    const double c00 = d * f - e * e, c01 = c * e - bb * f, c02 = bb * e - c * d;
    const double det = a * c00 + bb * c01 + c * c02;
    if (det < DET_MIN) return false;
    const double c11 = a * f - c * c, c12 = bb * c - a * e, c22 = a * d - bb * bb;
    const double r0 = s.bv[0] * iw, r1 = s.bv[1] * iw, r2 = s.bv[2] * iw, id = 1.0 / det;
    x[0] = cm[0] + (c00 * r0 + c01 * r1 + c02 * r2) * id;
    x[1] = cm[1] + (c01 * r0 + c11 * r1 + c12 * r2) * id;
    x[2] = cm[2] + (c02 * r0 + c12 * r1 + c22 * r2) * id;
    return true;
}

// squared distance of x to line v: the perpendicular part of x - c, formed as a vector
template <class Lines>
__device__ inline double line_dist2(const Lines& ln, int v, const double x[3]) {
    double u[3], t[3], uu = 0, ut = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double cc = ln.center(v, k);
        u[k] = ln.ray(v, k) - cc;
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
    return perp2;
}

// The confidence-weighted least-squares point of the views of `mask` that take part, and its weighted root-mean-square distance
// to them -- the one statement of that arithmetic, for triangulate_rays_kernel (every view) and for the refit of
// triangulate_robust_kernel (the inlier set).  False (x, res untouched): fewer than two such views, or a degenerate system.
template <class Lines>
__device__ inline bool weighted_point(const Lines& ln, int V, unsigned mask, double x[3], double& res) {
    // origin shift: the mean of the sample's camera centres (room-scale coordinates stay out of the normal equations)
    double cm[3] = {0, 0, 0};
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int d = 0; d < 3; ++d) cm[d] += ln.center(v, d);
#pragma unroll
    for (int d = 0; d < 3; ++d) cm[d] /= V;
    Normal s;
    int n = 0;
    for (int v = 0; v < V; ++v) {
        if (!(mask >> v & 1u)) continue;
        const double w = ln.weight(v);
        if (!takes_part(w)) continue;
        normal_add(s, ln, v, w, cm);
        ++n;
    }
    if (n < 2 || !normal_solve(s, cm, x)) return false;
    // residual on the lines themselves (second read of the same 24 V bytes, from the cache).  The one-pass form
    // sum w q^T M q - y^T b cancels to nothing exactly where the residual matters, at lines that nearly meet.
    double acc = 0;
    for (int v = 0; v < V; ++v) {
        if (!(mask >> v & 1u)) continue;
        const double w = ln.weight(v);
        if (!takes_part(w)) continue;
        acc += w * line_dist2(ln, v, x);
    }
    res = sqrt(acc * (1.0 / s.W));
    return true;
}

__global__ __launch_bounds__(256) void triangulate_rays_kernel(const GeoViews p, float* __restrict__ points,
                                                               float* __restrict__ residual) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)p.B * p.J) return;
    const GlobalLines ln{p, (size_t)(idx / p.J), (size_t)idx};
    const float nan = __builtin_nanf("");
    double x[3], res;
    const bool ok = weighted_point(ln, p.V, ~0u, x, res);
    float* po = points + (size_t)idx * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) po[k] = ok ? (float)x[k] : nan;
    residual[idx] = ok ? (float)res : nan;
}

// triangulate_robust_kernel: per (sample, joint) candidates -> pair consensus -> refit.  A workgroup stages the lines (and the
// confidences) of GEO_ITEMS items in LDS once; thread (wave s, lane it) scores the pairs s, s + ROBUST_WAVES, ... (in the i < k
// order of all V (V - 1) / 2 pairs) of item it and keeps its best in registers; the waves' bests meet in LDS and wave 0 refits
// and stores.  View sets are 32-bit masks (MPL_MAX_VIEWS = 32).  Eight waves: the scoring is a chain of dependent fp64
// operations on LDS operands, and a tile of 64 items is all a compute unit gets at the headline size, so the waves are what
// hides the latency (two per SIMD).
// LDS: lines [V][6][GEO_ITEMS] floats | conf [V][GEO_ITEMS] floats (with confidences) | best: cost [ROBUST_WAVES][GEO_ITEMS]
// doubles, then (count + 1) * 512 + pair and mask [ROBUST_WAVES][GEO_ITEMS] 32-bit words: 48 + 8 + 8 = 64 KiB at 32 views.
constexpr double ROBUST_CONF_THRESHOLD_MAX = 64.0;      // confidences are probabilities; the descent from 64 is 1300 steps
constexpr int ROBUST_WAVES = 8;
constexpr int ROBUST_BEST_BYTES = ROBUST_WAVES * GEO_ITEMS * (8 + 4 + 4);

__device__ inline bool better(int count, double cost, int pair, int bcount, double bcost, int bpair) {
    // the total order of the hypotheses: highest count, then lowest cost, then lowest i, then lowest k (= lowest pair index)
    return count > bcount || (count == bcount && (cost < bcost || (cost == bcost && pair < bpair)));
}

__global__ __launch_bounds__(GEO_ITEMS * ROBUST_WAVES) void triangulate_robust_kernel(const GeoViews p, double tau, double conf_th,
                                                                                    int min_inliers, float* __restrict__ points,
                                                                                    float* __restrict__ residual,
                                                                                    float* __restrict__ inliers) {
    extern __shared__ float lines[];
    const int tid = threadIdx.x, V = p.V;
    const bool has_conf = p.conf[0] != nullptr, tau_on = tau >= 0.0, conf_on = conf_th >= 0.0;     // NaN: off
    float* cf = lines + V * 6 * GEO_ITEMS;
    double* best_cost = reinterpret_cast<double*>(cf + (has_conf ? V * GEO_ITEMS : 0));
    int* best_key = reinterpret_cast<int*>(best_cost + ROBUST_WAVES * GEO_ITEMS);          // (count + 1) * 512 + pair
    unsigned* best_mask = reinterpret_cast<unsigned*>(best_key + ROBUST_WAVES * GEO_ITEMS);
    const long long total = (long long)p.B * p.J, first = (long long)blockIdx.x * GEO_ITEMS;
    const int items = (int)(total - first < GEO_ITEMS ? total - first : GEO_ITEMS);
    for (int e = tid; e < V * GEO_ITEMS * 3; e += GEO_ITEMS * ROBUST_WAVES) {
        const int v = e / (GEO_ITEMS * 3), t = e % (GEO_ITEMS * 3), it = t / 3, d = t % 3;
        if (it < items) {
            const long long idx = first + it;
            lines[(v * 6 + d) * GEO_ITEMS + it] = p.rays[v][(size_t)idx * 3 + d];
            lines[(v * 6 + 3 + d) * GEO_ITEMS + it] = p.centers[v][(size_t)(idx / p.J) * 3 + d];
        }
    }
    if (has_conf)
        for (int e = tid; e < V * GEO_ITEMS; e += GEO_ITEMS * ROBUST_WAVES) {
            const int v = e / GEO_ITEMS, it = e % GEO_ITEMS;
            if (it < items) cf[e] = p.conf[v][(size_t)(first + it) * p.conf_stride];
        }
    __syncthreads();
    const int it = tid % GEO_ITEMS, slice = tid / GEO_ITEMS;
    const bool live = it < items;
    const StagedLines ln{lines, has_conf ? cf : nullptr, it};

    // 1. candidates: the views that take part, and of those the ones triangulate.py:94-102 selects -- the threshold comes down
    // by 0.05 (repeated subtraction, the reference's bits) until two confidences exceed it or it is below -1.  Two confidences
    // exceed th exactly when the second largest does.
    unsigned cand = 0;
    if (live) {
        double c1 = -__builtin_inf(), c2 = -__builtin_inf();      // the two largest confidences (a NaN is never one)
        for (int v = 0; v < V; ++v) {
            const double w = ln.weight(v);
            if (takes_part(w)) cand |= 1u << v;
            if (w > c1) { c2 = c1; c1 = w; }
            else if (w > c2) c2 = w;
        }
        if (conf_on) {
            double th = conf_th;
            while (!(th < -1.0) && !(c2 > th)) th -= 0.05;
            unsigned sel = 0;
            for (int v = 0; v < V; ++v)
                if (ln.weight(v) > th) sel |= 1u << v;
            cand &= sel;
        }
    }

    // 2. consensus: every candidate pair is a hypothesis, the midpoint of the pair's common perpendicular
    int bcount = -1, bpair = 0;
    double bcost = 0;
    unsigned bmask = 0;
    if (tau_on) {
        const double tau2 = tau * tau;
        int pair = 0;
        for (int i = 0; i + 1 < V; ++i)
            for (int k = i + 1; k < V; ++k, ++pair) {
                if (pair % ROBUST_WAVES != slice) continue;          // wave-uniform
                if (!(cand >> i & cand >> k & 1u)) continue;
                double cm[3], x[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) cm[d] = 0.5 * (ln.center(i, d) + ln.center(k, d));
                Normal s;
                normal_add(s, ln, i, 1.0, cm);
                normal_add(s, ln, k, 1.0, cm);
                if (!normal_solve(s, cm, x)) continue;
                int count = 0;
                double cost = 0;
                unsigned mask = 0;
                for (int v = 0; v < V; ++v) {
                    if (!(cand >> v & 1u)) continue;
                    const double d2 = line_dist2(ln, v, x);
                    const bool in = d2 <= tau2;
                    cost += ln.weight(v) * (in ? d2 : tau2);
                    count += in;
                    mask |= (unsigned)in << v;
                }
                if (better(count, cost, pair, bcount, bcost, bpair)) {
                    bcount = count; bcost = cost; bpair = pair; bmask = mask;
                }
            }
        best_cost[tid] = bcost;
        best_key[tid] = (bcount + 1) * 512 + bpair;
        best_mask[tid] = bmask;
        __syncthreads();
    }
    if (slice != 0 || !live) return;
    unsigned inl = cand;
    bool ok = true;
    if (tau_on) {
        for (int s = 1; s < ROBUST_WAVES; ++s) {
            const int at = s * GEO_ITEMS + it, count = best_key[at] / 512 - 1, pair = best_key[at] % 512;
            if (better(count, best_cost[at], pair, bcount, bcost, bpair)) {
                bcount = count; bcost = best_cost[at]; bpair = pair; bmask = best_mask[at];
            }
        }
        ok = bcount >= min_inliers;          // no non-degenerate pair: -1
        inl = bmask;
    }

    // 3. refit on the inlier set
    double x[3], res;
    ok = ok && weighted_point(ln, V, inl, x, res);
    const long long idx = first + it;
    const size_t b = (size_t)(idx / p.J), j = (size_t)(idx % p.J);
    const float nan = __builtin_nanf("");
    float* po = points + (size_t)idx * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) po[k] = ok ? (float)x[k] : nan;
    residual[idx] = ok ? (float)res : nan;
    for (int v = 0; v < V; ++v) inliers[(b * V + v) * p.J + j] = ok && (inl >> v & 1u) ? 1.f : 0.f;
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

int launch_triangulate_robust(const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int B,
                              int V, int J, double threshold, double conf_threshold, int min_inliers, float* points,
                              float* residual, float* inliers, hipStream_t s) {
    GeoViews p;
    if (int rc = geo_views(p, rays, centers, conf, conf_stride, B, V, J, 1)) return rc;
    const bool conf_on = conf_threshold >= 0.0;          // negative or NaN: off
    if (!points || !residual || !inliers || (conf_on && !conf) || min_inliers < 2 || min_inliers > V) return MPL_E_INVALID;
    // the descent of the threshold is a loop of (conf_threshold + 1) / 0.05 steps in every thread
    if (conf_on && !(conf_threshold <= ROBUST_CONF_THRESHOLD_MAX)) return MPL_E_UNSUPPORTED;
    const long long total = (long long)B * J;
    const size_t lds = (size_t)V * (conf ? 7 : 6) * GEO_ITEMS * sizeof(float) + ROBUST_BEST_BYTES;      // 64 KiB at 32 views
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(triangulate_robust_kernel, dim3((unsigned)((total + GEO_ITEMS - 1) / GEO_ITEMS)), dim3(GEO_ITEMS * ROBUST_WAVES),
                       lds, s, p, threshold >= 0.0 ? threshold : -1.0, conf_on ? conf_threshold : -1.0, min_inliers, points, residual,
                       inliers);
    return hip_check_launch();
}

}  // namespace mpl
