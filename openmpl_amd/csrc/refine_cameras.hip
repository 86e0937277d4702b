// Refinement of camera poses by the reprojection error of known 3D points (mpl_refine_cameras): the transpose of refine.hip.
//
// refine.hip takes the rig as given and moves the points; this kernel takes the points as given and moves the cameras.  Per view v it
// minimises E_v(R, t) = sum_{b,j} w_bvj rho(|proj_v(X_bj) - px_bvj|^2) over the 6 unknowns of the pose by Levenberg-Marquardt, with
// the cost, the weights, the projection and the lens of refine.hip (camera_coords, distort_jet, f y_d + c of views.hpp); intrinsics and
// lens coefficients are not unknowns.  The reference has no such step.
//
// The parallel shape is the other one: not many small problems, one thread each, but at most 32 problems whose every evaluation is
// a reduction over all N = B J observations of the view.  One workgroup per view; the threads stride over the observations with fp64
// partial sums of E, the 21 entries of H and the 6 of g in registers; the sums go down each wave by shuffles and across the waves
// through LDS, in a fixed order and without atomics, so two runs give identical bits.  Thread 0 accepts or rejects the trial,
// factorises, forms the next trial pose and publishes it and a `done` word through LDS.  Every thread reaches every barrier: the
// loop ends only on that word, read by all threads after a barrier, and the trial count is bounded by max_iterations.
#include "common.hpp"
#include "reprojection.hpp"

namespace mpl {

namespace {

// 8 waves, two per SIMD: 256 registers a lane, which hold the 30 fp64 accumulators, the record, the lens jet and, in thread 0, the
// factorisation unrolled into registers (234 in all with a lens, no scratch, no spills); at B J = 17408 that is 34 observations per thread and
// evaluation
constexpr int RCAM_THREADS = 512, RCAM_WAVES = RCAM_THREADS / 64;
constexpr double RCAM_SMALL_ANGLE2 = 1e-8;

// What one evaluation at a pose leaves behind, as slots of an LDS row: the cost E in the mode of the call, the plain sum S = sum w
// |r|^2 and W = sum w (the error output), the normal equations H = sum w' J^T J (upper triangle, row-major) and g = sum w' J^T r, the
// count of observations that take part -- all sums --, the smallest depth and whether an observation that takes part is not in front
enum { RCAM_E = 0, RCAM_S = 1, RCAM_W = 2, RCAM_H = 3, RCAM_G = 24, RCAM_USED = 30, RCAM_SUMS = 31, RCAM_ZMIN = 31, RCAM_BEHIND = 32,
       RCAM_SLOTS = 33 };

struct RefineCamerasParams {
    const float* points;      // (B,J,3)
    const float* px;          // (B,V,J,2)
    const float* conf;        // (B,V,J) or null
    const double* cams;       // device (V,16)
    const double* dist;       // device (V,5) or null
    double* out_cams;         // (V,16); may be cams
    double* out_error;        // (V)
    double* out_cost0;        // (V) or null
    double* out_cost;         // (V) or null
    int* out_used;            // (V) or null
    int* out_iterations;      // (V) or null
    unsigned char* out_status;   // (V) or null
    double huber, tol;
    unsigned N, V, J, fixed_mask;             // N = B J observations per view; B V J <= 2^30
    int max_it;
};

// The sums of one thread over its observations of view v at the pose c (a camera record in registers).  LENS = false is the call
// without a distortion table: the zero coefficients are constants, and the polynomial folds to the pinhole.  normal = false (the same
// for the whole workgroup: a view that is passed through whatever it holds) leaves H and g at zero, which nobody reads then
template <bool LENS>
__device__ __forceinline__ void rcam_accumulate(const RefineCamerasParams& p, unsigned v, const double (&c)[16], const Distortion d, bool normal,
                                                double (&acc)[RCAM_USED], int& used, double& zmin, bool& behind) {
    const Camera cam{c};
    for (unsigned i = threadIdx.x; i < p.N; i += RCAM_THREADS) {
        const unsigned b = i / p.J, j = i - b * p.J;
        const unsigned o = (b * p.V + v) * p.J + j;            // below 2^30, so twice it fits 32 bits
        const double w = p.conf ? (double)p.conf[o] : 1.0;
        const float q0 = p.px[o * 2u], q1 = p.px[o * 2u + 1u];
        const float* x = p.points + (size_t)i * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        // takes part: a finite weight > 0, a finite pixel, a finite point
        if (!(takes_part(w) && isfinite(q0) && isfinite(q1) && isfinite(x0) && isfinite(x1) && isfinite(x2))) continue;
        ++used;
        double xc, yc, zc;
        camera_coords(c, (double)x0, (double)x1, (double)x2, xc, yc, zc);
        // not in front: flagged, and the sums go on with values nobody reads (the evaluation is dropped as a whole)
        behind |= !(zc > CAMERA_Z_MIN);
        zmin = fmin(zmin, zc);
        const double iz = 1.0 / zc, y0 = xc / zc, y1 = yc / zc;
        const LensJet jet = distort_jet(y0, y1, d);
        const double r0 = (cam.fx() * jet.x + cam.cx()) - (double)q0, r1 = (cam.fy() * jet.y + cam.cy()) - (double)q1;
        const double s = r0 * r0 + r1 * r1, rn = sqrt(s);
        // plain: rho(s) = s, w' = w.  Huber beyond h^2: rho(s) = 2 h sqrt(s) - h^2, w' = w h / |r| (the IRLS weight)
        const bool tail = p.huber > 0.0 && s > p.huber * p.huber;
        acc[RCAM_E] += w * (tail ? 2.0 * p.huber * rn - p.huber * p.huber : s);
        acc[RCAM_S] += w * s;
        acc[RCAM_W] += w;
        if (!normal) continue;
        const double wi = tail ? w * (p.huber / rn) : w;
        // M = d px / d x_cam = diag(f) (d y_d / d y) [1 0 -y0; 0 1 -y1] / z, and J = M [ -[x_cam]x | -R ] for R' = exp([w]x) R, t' = t + dt
        const double m00 = cam.fx() * jet.j00 * iz, m01 = cam.fx() * jet.j01 * iz, m02 = -(m00 * y0 + m01 * y1);
        const double m10 = cam.fy() * jet.j10 * iz, m11 = cam.fy() * jet.j11 * iz, m12 = -(m10 * y0 + m11 * y1);
        double a[6], bb[6];
        a[0] = m02 * yc - m01 * zc;
        a[1] = m00 * zc - m02 * xc;
        a[2] = m01 * xc - m00 * yc;
        bb[0] = m12 * yc - m11 * zc;
        bb[1] = m10 * zc - m12 * xc;
        bb[2] = m11 * xc - m10 * yc;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[3 + k] = -(m00 * cam.r(0, k) + m01 * cam.r(1, k) + m02 * cam.r(2, k));
            bb[3 + k] = -(m10 * cam.r(0, k) + m11 * cam.r(1, k) + m12 * cam.r(2, k));
        }
        int h = RCAM_H;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int l = k; l < 6; ++l) acc[h++] += wi * (a[k] * a[l] + bb[k] * bb[l]);
            acc[RCAM_G + k] += wi * (a[k] * r0 + bb[k] * r1);
        }
    }
}

// (H + lambda diag H) delta = -g by an unpivoted Cholesky factorisation; a pivot that is <= 0 or not finite gives a delta that is
// not a number, which no trial survives.  e: an evaluation's LDS row; everything else in registers, every index a constant
__device__ __forceinline__ void rcam_step(const double* e, double lambda, double (&delta)[6]) {
    double A[6][6], L[6][6], y[6];
    int h = RCAM_H;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int l = k; l < 6; ++l) A[k][l] = e[h++];
        A[k][k] = A[k][k] + lambda * A[k][k];
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
        ok = ok && dj > 0.0 && dj <= FINITE_MAX;
        L[j][j] = sqrt(dj);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = A[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {                         // L y = -g
        double s = -e[RCAM_G + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                        // L^T delta = y
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * delta[k];
        delta[i] = s / L[i][i];
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 6; ++i) delta[i] = __builtin_nan("");
    }
}

// the trial pose R' = exp([w]x) R, t' = t + dt from the accepted pose (R row-major, then t: 12 doubles); Rodrigues,
// exp([w]x) = I + a K + b K^2 with K^2 = w w^T - |w|^2 I
__device__ __forceinline__ void rcam_apply(const double* pose, const double (&delta)[6], double* trial) {
    const double w0 = delta[0], w1 = delta[1], w2 = delta[2], th2 = w0 * w0 + w1 * w1 + w2 * w2;
    double a, b;
    if (th2 < RCAM_SMALL_ANGLE2) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        double sn, cs;
        sincos(th, &sn, &cs);
        a = sn / th;
        b = (1.0 - cs) / th2;
    }
    const double ex[3][3] = {{1.0 + b * (w0 * w0 - th2), b * (w0 * w1) - a * w2, b * (w0 * w2) + a * w1},
                             {b * (w0 * w1) + a * w2, 1.0 + b * (w1 * w1 - th2), b * (w1 * w2) - a * w0},
                             {b * (w0 * w2) - a * w1, b * (w1 * w2) + a * w0, 1.0 + b * (w2 * w2 - th2)}};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) trial[3 * r + k] = ex[r][0] * pose[k] + ex[r][1] * pose[3 + k] + ex[r][2] * pose[6 + k];
        trial[9 + r] = pose[9 + r] + delta[3 + r];
    }
}

}  // namespace

template <bool LENS>
__global__ __launch_bounds__(RCAM_THREADS) void refine_cameras_kernel(const RefineCamerasParams p) {
    __shared__ double sh_part[RCAM_WAVES][RCAM_SLOTS];   // one row per wave
    __shared__ double sh_tr[RCAM_SLOTS];                 // the evaluation just made
    __shared__ double sh_cur[RCAM_SLOTS];                // the evaluation at the accepted pose (thread 0 only)
    __shared__ double sh_cam[21];                        // the record to evaluate: intrinsics, the trial pose, the lens row
    __shared__ double sh_pose[12];                       // the accepted pose (thread 0 only)
    __shared__ double sh_delta[6], sh_lambda, sh_E0;     // thread 0's state between the evaluations
    __shared__ int sh_done;
    const unsigned v = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;

    // The camera and lens records, read once, one entry per thread: a workgroup reads its row before it writes it and touches no
    // other row.  They go to the lanes through LDS and vector registers: as scalar loads their 42 registers, beside the kernel
    // arguments, no longer fit the scalar file
    if (tid < 16) sh_cam[tid] = p.cams[(size_t)v * 16 + tid];
    else if (LENS && tid < 21) sh_cam[tid] = p.dist[(size_t)v * 5 + (tid - 16)];
    __syncthreads();

    const bool fits = !(p.fixed_mask >> v & 1u) && p.max_it != 0;           // otherwise passed through, and scored only
    bool first = true;
    int status = LM_INVALID, trials = 0, used_out = 0;   // thread 0's

    // One call site of the evaluation: the first pass evaluates the given pose, every later one a trial pose
    for (;;) {
        double c[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = sh_cam[k];
        const Distortion d = distortion_from<LENS>(sh_cam + 16);
        double acc[RCAM_USED], zmin = __builtin_inf();
#pragma unroll
        for (int k = 0; k < RCAM_USED; ++k) acc[k] = 0.0;
        int used = 0;
        bool behind = false;
        rcam_accumulate<LENS>(p, v, c, d, fits, acc, used, zmin, behind);

        // down each wave by shuffles, in a fixed order ...
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < RCAM_USED; ++k) acc[k] += __shfl_down(acc[k], off, 64);
            used += __shfl_down(used, off, 64);
            zmin = fmin(zmin, __shfl_down(zmin, off, 64));
        }
        const bool wave_behind = __any(behind);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < RCAM_USED; ++k) sh_part[wave][k] = acc[k];
            sh_part[wave][RCAM_USED] = (double)used;
            sh_part[wave][RCAM_ZMIN] = zmin;
            sh_part[wave][RCAM_BEHIND] = wave_behind ? 1.0 : 0.0;
        }
        __syncthreads();
        // ... then across the waves in the order of the waves, one slot per thread
        if (tid < RCAM_SLOTS) {
            double r = sh_part[0][tid];
            for (int w = 1; w < RCAM_WAVES; ++w) {
                const double o = sh_part[w][tid];
                r = tid < RCAM_SUMS ? r + o : tid == RCAM_ZMIN ? fmin(r, o) : fmax(r, o);
            }
            sh_tr[tid] = r;
        }
        __syncthreads();

        if (tid == 0) {
            bool done = false, accept = false;
            if (first) {
                used_out = (int)sh_tr[RCAM_USED];
                bool valid = used_out > 0 && sh_tr[RCAM_BEHIND] == 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k) valid = valid && fabs(c[k]) <= FINITE_MAX;
#pragma unroll
                for (int k = 0; k < 12; ++k) sh_pose[k] = c[4 + k];
                if (!valid) {
                    done = true;                                              // LM_INVALID
                } else {
                    accept = true;
                    sh_E0 = sh_tr[RCAM_E];
                    sh_lambda = LM_LAMBDA0;
                    status = LM_PASSED_THROUGH;
                    if (!fits || used_out < 3) done = true;
                    else status = LM_CAPPED;
                }
            } else {
                ++trials;
                // strictly lower and everything in front; a cost that is not a number is never accepted
                accept = sh_tr[RCAM_BEHIND] == 0.0 && sh_tr[RCAM_E] < sh_cur[RCAM_E];
                if (accept) {
                    for (int k = 0; k < 12; ++k) sh_pose[k] = sh_cam[4 + k];
                    sh_lambda = fmax(sh_lambda / 10.0, LM_LAMBDA_MIN);
                } else {
                    sh_lambda = sh_lambda * 10.0;
                }
            }
            if (accept) {
                for (int k = 0; k < RCAM_SLOTS; ++k) sh_cur[k] = sh_tr[k];
            }
            if (!first) {
                const double tt = p.tol * sh_cur[RCAM_ZMIN];
                bool small = true;                                            // a step that is not a number is below nothing
                for (int k = 0; k < 6; ++k) small = small && fabs(sh_delta[k]) <= (k < 3 ? p.tol : tt);
                if (small) {
                    status = LM_CONVERGED;
                    done = true;
                } else if (sh_lambda > LM_LAMBDA_MAX || trials >= p.max_it) {
                    done = true;
                }
            }
            if (!done) {
                double delta[6];
                rcam_step(sh_cur, sh_lambda, delta);
                rcam_apply(sh_pose, delta, sh_cam + 4);
#pragma unroll
                for (int k = 0; k < 6; ++k) sh_delta[k] = delta[k];
            }
            sh_done = done ? 1 : 0;
        }
        __syncthreads();
        if (sh_done) break;                               // the same word for every thread
        first = false;
    }

    if (tid == 0) {
        // Intrinsics as given; the pose the last accepted one, which is the given row's bits where nothing was accepted -- passed
        // through or invalid: a row that is not a number would poison every later call, so it is handed back, not replaced
        const double nan = __builtin_nan("");
        const bool valid = status != LM_INVALID;
        double* row = p.out_cams + (size_t)v * 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) row[k] = sh_cam[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) row[4 + k] = sh_pose[k];
        p.out_error[v] = valid ? sqrt(sh_cur[RCAM_S] / sh_cur[RCAM_W]) : nan;
        if (p.out_cost0) p.out_cost0[v] = valid ? sh_E0 : nan;
        if (p.out_cost) p.out_cost[v] = valid ? sh_cur[RCAM_E] : nan;
        if (p.out_used) p.out_used[v] = used_out;
        if (p.out_iterations) p.out_iterations[v] = trials;
        if (p.out_status) p.out_status[v] = (unsigned char)status;
    }
}

int launch_refine_cameras(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                          int B, int V, int J, double huber, int max_iterations, double step_tolerance, unsigned fixed_mask,
                          double* out_cams, double* out_error, double* out_cost0, double* out_cost, int* out_used, int* out_iterations,
                          unsigned char* out_status, hipStream_t s) {
    if (const int e = refine_args_check(points, pixels, cams_dev, out_cams, out_error, B, V, J, max_iterations, step_tolerance)) return e;
    RefineCamerasParams p;
    p.points = points; p.px = pixels; p.conf = conf; p.cams = cams_dev; p.dist = dist_dev;
    p.out_cams = out_cams; p.out_error = out_error; p.out_cost0 = out_cost0; p.out_cost = out_cost; p.out_used = out_used;
    p.out_iterations = out_iterations; p.out_status = out_status;
    p.huber = huber > 0.0 ? huber : 0.0;                 // <= 0 or NaN: the plain cost
    p.tol = step_tolerance;
    p.N = (unsigned)(B * J); p.V = (unsigned)V; p.J = (unsigned)J; p.fixed_mask = fixed_mask; p.max_it = max_iterations;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dist_dev)
        hipLaunchKernelGGL(refine_cameras_kernel<true>, dim3((unsigned)V), dim3(RCAM_THREADS), 0, s, p);
    else
        hipLaunchKernelGGL(refine_cameras_kernel<false>, dim3((unsigned)V), dim3(RCAM_THREADS), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
