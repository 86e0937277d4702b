// Refinement of 3D points by their reprojection error, and the reprojection error of any 3D estimate (mpl_refine_points).
//
// The triangulations of geometry.hip minimise the distance to the lines of sight in world units; a detector errs in pixels, and a
// camera twice as far away turns the same pixel error into twice the ray distance.  This kernel minimises
// E(X) = sum_v w_v rho(|proj_v(X) - px_v|^2) by Levenberg-Marquardt on the 3 unknowns of a point, from the point it is given.  The
// reference has no such step.  The projection is that of project_points(distortion=): camera_coords, distort_normalized (here
// through distort_jet, which adds the Jacobian), f y_d + c -- all of views.hpp.
//
// One work item = one (sample, joint); one thread per item, the views in a wave-uniform loop, so the camera and lens records are
// wave-uniform loads.  fp64 on the fp32 tensors, every output rounded once, no LDS, no atomics, the sum over the views in the order
// of the views: identical bits from run to run and from batching to batching.  Workgroups of one wave: at the headline size
// (1024 x 17 items) that is about one wave per compute unit, and the kernel is a chain of dependent fp64 operations per lane.
#include "common.hpp"
#include "reprojection.hpp"

namespace mpl {

namespace {

constexpr int REFINE_THREADS = 64;

struct RefineParams {
    const float* points;      // (B,J,3)
    const float* px;          // (B,V,J,2)
    const float* conf;        // (B,V,J) or null
    const double* cams;       // device (V,16)
    const double* dist;       // device (V,5) or null
    float* out_points;        // (B,J,3)
    float* out_error;         // (B,J)
    float* out_errors;        // (B,V,J) or null
    int* out_iterations;      // (B,J) or null
    unsigned char* out_status;   // (B,J) or null
    double huber, tol;
    int total, V, J, max_it;
};

// the item's view of its inputs: view v of item (b, j) sits at element (b V + v) J + j
struct RefineItem {
    const RefineParams& p;
    unsigned base;            // b V J + j; batch * views * joints <= 2^30, so an observation's index (and twice it) fits 32 bits
    __device__ unsigned at(int v) const { return base + (unsigned)(v * p.J); }
    __device__ double weight(int v) const { return p.conf ? (double)p.conf[at(v)] : 1.0; }
};

// what one evaluation at X leaves behind: the cost E in the mode of the call, the normal equations
// H = sum w' J^T J (xx xy xz yy yz zz), g = sum w' J^T r, the smallest depth, and whether a view that takes part has X behind it
struct RefineEval {
    double E = 0, H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, zmin = __builtin_inf();
    bool behind = false;
};

// r = proj_v(X) - px_v in pixels and the lens jet at the point; false: z_cam <= CAMERA_Z_MIN (or not a number).  LENS = false is
// the call without a distortion table: the zero coefficients are constants, and the polynomial folds to the pinhole
template <bool LENS>
__device__ __forceinline__ bool refine_residual(const RefineItem& it, int v, const double X[3], double& r0, double& r1, double& y0,
                                                double& y1, double& zc, LensJet& jet) {
    const double* c = it.p.cams + (size_t)v * 16;
    const Camera cam{c};
    double xc, yc;
    camera_coords(c, X[0], X[1], X[2], xc, yc, zc);
    y0 = xc / zc;
    y1 = yc / zc;
    // The lens record goes through vector registers: its row is addressed with a per-lane zero the compiler cannot see through
    // (an observation's index is below 2^30).  As scalar loads its 10 registers, beside the 32 of the camera record, the kernel
    // arguments and the masks of three nested loops, no longer fit the scalar file, and the compiler spills.
    jet = distort_jet(y0, y1, distortion_of(LENS ? it.p.dist : nullptr, v + (int)(it.base >> 30)));
    const float* q = it.p.px + it.at(v) * 2u;
    r0 = (cam.fx() * jet.x + cam.cx()) - (double)q[0];
    r1 = (cam.fy() * jet.y + cam.cy()) - (double)q[1];
    return zc > CAMERA_Z_MIN;
}

template <bool LENS>
__device__ __forceinline__ RefineEval refine_eval(const RefineItem& it, unsigned mask, const double X[3], double huber) {
    RefineEval e;
    for (int v = 0; v < it.p.V; ++v) {
        if (!(mask >> v & 1u)) continue;
        double r0, r1, y0, y1, zc;
        LensJet jet;
        // behind the camera: flagged, and the sums go on with values nobody reads (the caller drops the whole evaluation)
        e.behind |= !refine_residual<LENS>(it, v, X, r0, r1, y0, y1, zc, jet);
        e.zmin = fmin(e.zmin, zc);
        const Camera cam{it.p.cams + (size_t)v * 16};
        const double w = it.weight(v), s = r0 * r0 + r1 * r1;
        // plain: rho(s) = s, w' = w.  Huber beyond h^2: rho(s) = 2 h sqrt(s) - h^2, w' = w h / |r| (the IRLS weight)
        const double rn = sqrt(s);
        const bool tail = huber > 0.0 && s > huber * huber;
        e.E += w * (tail ? 2.0 * huber * rn - huber * huber : s);
        const double wi = tail ? w * (huber / rn) : w;
        // J = diag(f) (d y_d / d y) (d y / d x_cam) R, with d y / d x_cam = [1 0 -y0; 0 1 -y1] / z
        const double iz = 1.0 / zc;
        const double m00 = cam.fx() * jet.j00 * iz, m01 = cam.fx() * jet.j01 * iz, m02 = -(m00 * y0 + m01 * y1);
        const double m10 = cam.fy() * jet.j10 * iz, m11 = cam.fy() * jet.j11 * iz, m12 = -(m10 * y0 + m11 * y1);
        double a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = m00 * cam.r(0, k) + m01 * cam.r(1, k) + m02 * cam.r(2, k);
            b[k] = m10 * cam.r(0, k) + m11 * cam.r(1, k) + m12 * cam.r(2, k);
        }
        e.H[0] += wi * (a[0] * a[0] + b[0] * b[0]);
        e.H[1] += wi * (a[0] * a[1] + b[0] * b[1]);
        e.H[2] += wi * (a[0] * a[2] + b[0] * b[2]);
        e.H[3] += wi * (a[1] * a[1] + b[1] * b[1]);
        e.H[4] += wi * (a[1] * a[2] + b[1] * b[2]);
        e.H[5] += wi * (a[2] * a[2] + b[2] * b[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) e.g[k] += wi * (a[k] * r0 + b[k] * r1);
    }
    return e;
}

// (H + lambda diag H) delta = -g by the adjugate; a singular system gives a delta that is not finite, which no trial survives
__device__ __forceinline__ void refine_step(const RefineEval& e, double lambda, double delta[3]) {
    const double a = e.H[0] + lambda * e.H[0], bb = e.H[1], c = e.H[2], d = e.H[3] + lambda * e.H[3], f = e.H[4], h = e.H[5] + lambda * e.H[5];
    const double c00 = d * h - f * f, c01 = c * f - bb * h, c02 = bb * f - c * d;
    const double c11 = a * h - c * c, c12 = bb * c - a * f, c22 = a * d - bb * bb;
    const double id = -1.0 / (a * c00 + bb * c01 + c * c02);
    delta[0] = (c00 * e.g[0] + c01 * e.g[1] + c02 * e.g[2]) * id;
    delta[1] = (c01 * e.g[0] + c11 * e.g[1] + c12 * e.g[2]) * id;
    delta[2] = (c02 * e.g[0] + c12 * e.g[1] + c22 * e.g[2]) * id;
}

}  // namespace

template <bool LENS>
__global__ __launch_bounds__(REFINE_THREADS) void refine_points_kernel(const RefineParams p) {
    const int idx = blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (idx >= p.total) return;
    const int V = p.V, b = idx / p.J, j = idx % p.J;
    const RefineItem it{p, (unsigned)(b * V * p.J + j)};
    const float nan = __builtin_nanf("");
    const float x0 = p.points[(size_t)idx * 3], x1 = p.points[(size_t)idx * 3 + 1], x2 = p.points[(size_t)idx * 3 + 2];
    double X[3] = {(double)x0, (double)x1, (double)x2};

    // the views that take part: a finite weight > 0 and two finite pixel coordinates
    unsigned mask = 0;
    int n = 0;
    for (int v = 0; v < V; ++v) {
        const double w = it.weight(v);
        const float* q = p.px + it.at(v) * 2u;
        const bool in = takes_part(w) && isfinite(q[0]) && isfinite(q[1]);
        mask |= (unsigned)in << v;
        n += in;
    }
    // One call site of the evaluation: the first pass of the loop evaluates the given point, every later one a trial step.
    RefineEval cur;
    bool valid = isfinite(x0) && isfinite(x1) && isfinite(x2) && n > 0, first = true;
    int status = LM_INVALID, trials = 0;
    double lambda = LM_LAMBDA0, Xt[3] = {X[0], X[1], X[2]}, delta[3] = {0, 0, 0};
    while (valid) {
        const RefineEval tr = refine_eval<LENS>(it, mask, Xt, p.huber);
        if (first) {
            first = false;
            valid = !tr.behind;
            if (!valid) break;
            cur = tr;
            status = LM_PASSED_THROUGH;
            if (n < 2 || p.max_it == 0) break;
            status = LM_CAPPED;
        } else {
            ++trials;
            if (!tr.behind && tr.E < cur.E) {            // strictly lower; a cost that is not a number is never accepted
                cur = tr;
#pragma unroll
                for (int k = 0; k < 3; ++k) X[k] = Xt[k];
                lambda = fmax(lambda / 10.0, LM_LAMBDA_MIN);
            } else {
                lambda *= 10.0;
            }
            if (fmax(fabs(delta[0]), fmax(fabs(delta[1]), fabs(delta[2]))) <= p.tol * cur.zmin) {
                status = LM_CONVERGED;
                break;
            }
            if (lambda > LM_LAMBDA_MAX || trials >= p.max_it) break;
        }
        refine_step(cur, lambda, delta);
#pragma unroll
        for (int k = 0; k < 3; ++k) Xt[k] = X[k] + delta[k];
    }

    // the errors at the final point: |r_v| per view, and the plain weighted root mean square in both modes
    double S = 0, W = 0;
    for (int v = 0; v < V; ++v) {
        float ev = nan;
        if (valid && (mask >> v & 1u)) {
            double r0, r1, y0, y1, zc;
            LensJet jet;
            refine_residual<LENS>(it, v, X, r0, r1, y0, y1, zc, jet);       // in front: the final point has a finite cost
            const double s = r0 * r0 + r1 * r1, w = it.weight(v);
            S += w * s;
            W += w;
            ev = (float)sqrt(s);
        }
        if (p.out_errors) p.out_errors[it.at(v)] = ev;
    }
    float* po = p.out_points + (size_t)idx * 3;
    // passed through, or no trial accepted: X still holds the input's bits
    po[0] = valid ? (float)X[0] : nan;
    po[1] = valid ? (float)X[1] : nan;
    po[2] = valid ? (float)X[2] : nan;
    p.out_error[idx] = valid ? (float)sqrt(S / W) : nan;
    if (p.out_iterations) p.out_iterations[idx] = trials;
    if (p.out_status) p.out_status[idx] = (unsigned char)status;
}

int launch_refine_points(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                         int B, int V, int J, double huber, int max_iterations, double step_tolerance, float* out_points,
                         float* out_error, float* out_errors, int* out_iterations, unsigned char* out_status, hipStream_t s) {
    if (const int e = refine_args_check(points, pixels, cams_dev, out_points, out_error, B, V, J, max_iterations, step_tolerance)) return e;
    RefineParams p;
    p.points = points; p.px = pixels; p.conf = conf; p.cams = cams_dev; p.dist = dist_dev;
    p.out_points = out_points; p.out_error = out_error; p.out_errors = out_errors; p.out_iterations = out_iterations;
    p.out_status = out_status;
    p.huber = huber > 0.0 ? huber : 0.0;                 // <= 0 or NaN: the plain cost
    p.tol = step_tolerance;
    p.total = B * J; p.V = V; p.J = J; p.max_it = max_iterations;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    const dim3 grid((unsigned)((p.total + REFINE_THREADS - 1) / REFINE_THREADS));
    if (dist_dev)
        hipLaunchKernelGGL(refine_points_kernel<true>, grid, dim3(REFINE_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(refine_points_kernel<false>, grid, dim3(REFINE_THREADS), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
