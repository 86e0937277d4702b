// The polish of a relative pose (mpl_refine_relative_pose): Levenberg-Marquardt on the 5 unknowns of (R, t), |t| = 1, over the signed
// Sampson distances of the correspondences of a pair.
//
// relative_pose.hip finds a pose within a few degrees; alternating bundle adjustment crawls along the two-view valley from there.  This
// kernel is the loop of refine_cameras.hip -- lambda policy, strict-decrease acceptance, statuses, the constants of reprojection.hpp --
// on the residual of step 4 of mpl_relative_pose: d = u_b^T F u_a / |gradient| with F = K_b^-T [t]x R K_a^-1.  With the normalised
// points a = K_a^-1 u_a, b = K_b^-1 u_b and E = [t]x R, d = n / s with n = b^T E a and s^2 = (E a)_0^2 / fxb^2 + (E a)_1^2 / fyb^2 +
// (E^T b)_0^2 / fxa^2 + (E^T b)_1^2 / fya^2: n and the four gradient entries are linear in E, so the derivative of d along a direction
// E' of E is n' / s - n (g . g') / s^3, analytic.  A trial is R' = exp([w]x) R, t' = normalise(t + d1 e1 + d2 e2); the five directions
// are [t]x [e_k]x R (k = 0 .. 2) and [e_i]x R (i = 1, 2).  One workgroup per pair, the sums in fp64 down the waves and across them in
// a fixed order, no atomics; thread 0 accepts or rejects, factorises and publishes the next trial, as in refine_cameras.hip.
#include "common.hpp"
#include "reprojection.hpp"

namespace mpl {

namespace {

constexpr int RREL_THREADS = 256, RREL_WAVES = RREL_THREADS / 64;
constexpr int RREL_MIN = 6;              // fewer participants than this: passed through
constexpr double RREL_SMALL_ANGLE2 = 1e-8;
// an evaluation's LDS row: E in the mode of the call, S = sum w d^2, W = sum w, H (upper triangle, row-major), g, the count
enum { RREL_E = 0, RREL_S = 1, RREL_W = 2, RREL_H = 3, RREL_G = 18, RREL_USED = 23, RREL_SLOTS = 24 };

struct RefineRelativeParams {
    const float* px;          // (B,V,J,2)
    const float* conf;        // (B,V,J) or null
    const float* weight;      // (B,P,J) or null
    const double* cams;       // device (V,16)
    const double* dist;       // device (V,5) or null
    const double* rotation;   // (P,9)
    const double* direction;  // (P,3)
    double* out_rotation;     // (P,9)
    double* out_direction;    // (P,3)
    double* out_cams;         // (P,2,16)
    double* out_error;        // (P)
    double* out_cost0;        // (P) or null
    double* out_cost;         // (P) or null
    int* out_used;            // (P) or null
    int* out_iterations;      // (P) or null
    unsigned char* out_status;   // (P) or null
    double huber, tol, baseline;
    unsigned N, V, J, P;
    int max_it;
    unsigned char va[MPL_MAX_VIEWS], vb[MPL_MAX_VIEWS];
};

// the tangent plane at t: e1 = normalise(t x axis_k), k the coordinate of t of the smallest magnitude (the lowest among equals),
// e2 = t x e1
__device__ __forceinline__ void rrel_tangent(const double* t, double (&e1)[3], double (&e2)[3]) {
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
    const double ax[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double c[3] = {t[1] * ax[2] - t[2] * ax[1], t[2] * ax[0] - t[0] * ax[2], t[0] * ax[1] - t[1] * ax[0]};
    const double n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) e1[i] = c[i] / n;
    e2[0] = t[1] * e1[2] - t[2] * e1[1];
    e2[1] = t[2] * e1[0] - t[0] * e1[2];
    e2[2] = t[0] * e1[1] - t[1] * e1[0];
}

// M = [v]x A for a 3 x 3 A (row-major)
__device__ __forceinline__ void rrel_cross_mat(const double* v, const double* A, double* M) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        M[c] = v[1] * A[6 + c] - v[2] * A[3 + c];
        M[3 + c] = v[2] * A[c] - v[0] * A[6 + c];
        M[6 + c] = v[0] * A[3 + c] - v[1] * A[c];
    }
}

// n = b^T M a and the four gradient entries of a 3 x 3 M at one correspondence; k: 1/fxb, 1/fyb, 1/fxa, 1/fya
__device__ __forceinline__ void rrel_forms(const double* M, double a0, double a1, double b0, double b1, const double (&k)[4], double& n,
                                           double (&g)[4]) {
    const double m0 = M[0] * a0 + M[1] * a1 + M[2], m1 = M[3] * a0 + M[4] * a1 + M[5], m2 = M[6] * a0 + M[7] * a1 + M[8];
    n = b0 * m0 + b1 * m1 + m2;
    g[0] = m0 * k[0];
    g[1] = m1 * k[1];
    g[2] = (M[0] * b0 + M[3] * b1 + M[6]) * k[2];
    g[3] = (M[1] * b0 + M[4] * b1 + M[7]) * k[3];
}

// (H + lambda diag H) delta = -g by an unpivoted Cholesky factorisation; a pivot that is <= 0 or not finite gives a NaN step
__device__ __forceinline__ void rrel_step(const double* e, double lambda, double (&delta)[5]) {
    double A[5][5], L[5][5], y[5];
    int h = RREL_H;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int l = k; l < 5; ++l) A[k][l] = e[h++];
        A[k][k] = A[k][k] + lambda * A[k][k];
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
        ok = ok && dj > 0.0 && dj <= FINITE_MAX;
        L[j][j] = sqrt(dj);
#pragma unroll
        for (int i = j + 1; i < 5; ++i) {
            double s = A[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double s = -e[RREL_G + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 5; ++k) s -= L[k][i] * delta[k];
        delta[i] = s / L[i][i];
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 5; ++i) delta[i] = __builtin_nan("");
    }
}

// the trial pose from the accepted one (R row-major, then t): R' = exp([w]x) R by Rodrigues, t' = normalise(t + d1 e1 + d2 e2)
__device__ __forceinline__ void rrel_apply(const double* pose, const double (&delta)[5], double* trial) {
    const double w0 = delta[0], w1 = delta[1], w2 = delta[2], th2 = w0 * w0 + w1 * w1 + w2 * w2;
    double a, b;
    if (th2 < RREL_SMALL_ANGLE2) {
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
    double e1[3], e2[3], t[3];
    rrel_tangent(pose + 9, e1, e2);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) trial[3 * r + k] = ex[r][0] * pose[k] + ex[r][1] * pose[3 + k] + ex[r][2] * pose[6 + k];
        t[r] = pose[9 + r] + delta[3] * e1[r] + delta[4] * e2[r];
    }
    const double n = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) trial[9 + r] = t[r] / n;
}

}  // namespace

template <bool LENS>
__global__ __launch_bounds__(RREL_THREADS) void refine_relative_kernel(const RefineRelativeParams p) {
    __shared__ double sh_part[RREL_WAVES][RREL_SLOTS], sh_tr[RREL_SLOTS], sh_cur[RREL_SLOTS];
    __shared__ double sh_cam[2][21];
    __shared__ double sh_trial[12], sh_pose[12], sh_delta[5], sh_lambda, sh_E0;
    __shared__ int sh_done;
    const unsigned q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned va = p.va[q], vb = p.vb[q];
    if (tid < 64) {
        const unsigned side = tid >> 5, k = tid & 31u, v = side ? vb : va;
        if (k < 16) sh_cam[side][k] = p.cams[(size_t)v * 16 + k];
        else if (LENS && k < 21) sh_cam[side][k] = p.dist[(size_t)v * 5 + (k - 16)];
    } else if (tid < 64 + 9) {
        sh_trial[tid - 64] = p.rotation[(size_t)q * 9 + (tid - 64)];
    } else if (tid < 64 + 12) {
        sh_trial[tid - 64] = p.direction[(size_t)q * 3 + (tid - 64 - 9)];
    }
    __syncthreads();
    double ca[16], cb[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        ca[k] = sh_cam[0][k];
        cb[k] = sh_cam[1][k];
    }
    const Distortion da = distortion_from<LENS>(sh_cam[0] + 16), db = distortion_from<LENS>(sh_cam[1] + 16);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) finite = finite && fabs(ca[k]) <= FINITE_MAX && fabs(cb[k]) <= FINITE_MAX;
    const double kk[4] = {1.0 / cb[0], 1.0 / cb[1], 1.0 / ca[0], 1.0 / ca[1]};
    const bool fits = p.max_it != 0;
    bool first = true;
    int status = LM_INVALID, trials = 0, used_out = 0;   // thread 0's

    for (;;) {
        // the pose to evaluate, E = [t]x R and its five directions
        double pose[12], M[6][9];
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = sh_trial[k];
        rrel_cross_mat(pose + 9, pose, M[0]);
        {
            double e1[3], e2[3], T[9];
            rrel_tangent(pose + 9, e1, e2);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double ax[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
                rrel_cross_mat(ax, pose, T);
                rrel_cross_mat(pose + 9, T, M[1 + k]);
            }
            rrel_cross_mat(e1, pose, M[4]);
            rrel_cross_mat(e2, pose, M[5]);
        }
        double acc[RREL_USED];
#pragma unroll
        for (int k = 0; k < RREL_USED; ++k) acc[k] = 0.0;
        int used = 0;
        for (unsigned i = tid; i < p.N; i += RREL_THREADS) {
            const unsigned b = i / p.J, j = i - b * p.J;
            const unsigned oa = (b * p.V + va) * p.J + j, ob = (b * p.V + vb) * p.J + j;
            const double wa = p.conf ? (double)p.conf[oa] : 1.0, wb = p.conf ? (double)p.conf[ob] : 1.0;
            const double wp = p.weight ? (double)p.weight[((size_t)b * p.P + q) * p.J + j] : 1.0;
            const float qa0 = p.px[oa * 2u], qa1 = p.px[oa * 2u + 1u], qb0 = p.px[ob * 2u], qb1 = p.px[ob * 2u + 1u];
            if (!(finite && takes_part(wa) && takes_part(wb) && takes_part(wp) && isfinite(qa0) && isfinite(qa1) && isfinite(qb0) &&
                  isfinite(qb1)))
                continue;
            double ua0, ua1, ub0, ub1;
            if (!undistort_pixel(ca, da, (double)qa0, (double)qa1, ua0, ua1)) continue;
            if (!undistort_pixel(cb, db, (double)qb0, (double)qb1, ub0, ub1)) continue;
            ++used;
            const double w = wa * wb * wp;
            const double a0 = (ua0 - ca[2]) / ca[0], a1 = (ua1 - ca[3]) / ca[1], b0 = (ub0 - cb[2]) / cb[0], b1 = (ub1 - cb[3]) / cb[1];
            double n, g[4];
            rrel_forms(M[0], a0, a1, b0, b1, kk, n, g);
            const double s2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3], s = sqrt(s2);
            const double d = n / s, dd = d * d, ad = fabs(d);
            const bool tail = p.huber > 0.0 && dd > p.huber * p.huber;
            acc[RREL_E] += w * (tail ? 2.0 * p.huber * ad - p.huber * p.huber : dd);
            acc[RREL_S] += w * dd;
            acc[RREL_W] += w;
            if (!fits) continue;
            const double wi = tail ? w * (p.huber / ad) : w;
            double jac[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                double nk, gk[4];
                rrel_forms(M[1 + k], a0, a1, b0, b1, kk, nk, gk);
                jac[k] = nk / s - n * (g[0] * gk[0] + g[1] * gk[1] + g[2] * gk[2] + g[3] * gk[3]) / (s2 * s);
            }
            int h = RREL_H;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
#pragma unroll
                for (int l = k; l < 5; ++l) acc[h++] += wi * (jac[k] * jac[l]);
                acc[RREL_G + k] += wi * (jac[k] * d);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < RREL_USED; ++k) acc[k] += __shfl_down(acc[k], off, 64);
            used += __shfl_down(used, off, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < RREL_USED; ++k) sh_part[wave][k] = acc[k];
            sh_part[wave][RREL_USED] = (double)used;
        }
        __syncthreads();
        if (tid < RREL_SLOTS) {
            double r = sh_part[0][tid];
            for (int w = 1; w < RREL_WAVES; ++w) r += sh_part[w][tid];
            sh_tr[tid] = r;
        }
        __syncthreads();

        if (tid == 0) {
            bool done = false, accept = false;
            if (first) {
                used_out = (int)sh_tr[RREL_USED];
                bool valid = used_out > 0 && sh_tr[RREL_E] <= FINITE_MAX;
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    valid = valid && fabs(pose[k]) <= FINITE_MAX;
                    sh_pose[k] = pose[k];
                }
                if (!valid) {
                    done = true;                                              // LM_INVALID
                } else {
                    accept = true;
                    sh_E0 = sh_tr[RREL_E];
                    sh_lambda = LM_LAMBDA0;
                    status = LM_PASSED_THROUGH;
                    if (!fits || used_out < RREL_MIN) done = true;
                    else status = LM_CAPPED;
                }
            } else {
                ++trials;
                accept = sh_tr[RREL_E] < sh_cur[RREL_E];      // strictly lower; a cost that is not a number is never accepted
                if (accept) {
                    for (int k = 0; k < 12; ++k) sh_pose[k] = sh_trial[k];
                    sh_lambda = fmax(sh_lambda / 10.0, LM_LAMBDA_MIN);
                } else {
                    sh_lambda = sh_lambda * 10.0;
                }
            }
            if (accept) {
                for (int k = 0; k < RREL_SLOTS; ++k) sh_cur[k] = sh_tr[k];
            }
            if (!first) {
                bool small = true;                                            // a step that is not a number is below nothing
                for (int k = 0; k < 5; ++k) small = small && fabs(sh_delta[k]) <= p.tol;
                if (small) {
                    status = LM_CONVERGED;
                    done = true;
                } else if (sh_lambda > LM_LAMBDA_MAX || trials >= p.max_it) {
                    done = true;
                }
            }
            if (!done) {
                double delta[5];
                rrel_step(sh_cur, sh_lambda, delta);
                rrel_apply(sh_pose, delta, sh_trial);
#pragma unroll
                for (int k = 0; k < 5; ++k) sh_delta[k] = delta[k];
            }
            sh_done = done ? 1 : 0;
        }
        __syncthreads();
        if (sh_done) break;                               // the same word for every thread
        first = false;
    }

    if (tid == 0) {
        const double nan = __builtin_nan("");
        const bool valid = status != LM_INVALID;
        double* ra = p.out_cams + (size_t)q * 32;
        double* rb = ra + 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ra[k] = sh_cam[0][k];
            rb[k] = sh_cam[1][k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            ra[4 + k] = valid ? ((k % 4 == 0) ? 1.0 : 0.0) : nan;
            rb[4 + k] = valid ? sh_pose[k] : nan;
            p.out_rotation[(size_t)q * 9 + k] = sh_pose[k];       // the given bits where nothing was accepted
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ra[13 + k] = valid ? 0.0 : nan;
            rb[13 + k] = valid ? -(p.baseline * (sh_pose[k] * sh_pose[9] + sh_pose[3 + k] * sh_pose[10] + sh_pose[6 + k] * sh_pose[11])) : nan;
            p.out_direction[(size_t)q * 3 + k] = sh_pose[9 + k];
        }
        p.out_error[q] = valid ? sqrt(sh_cur[RREL_S] / sh_cur[RREL_W]) : nan;
        if (p.out_cost0) p.out_cost0[q] = valid ? sh_E0 : nan;
        if (p.out_cost) p.out_cost[q] = valid ? sh_cur[RREL_E] : nan;
        if (p.out_used) p.out_used[q] = used_out;
        if (p.out_iterations) p.out_iterations[q] = trials;
        if (p.out_status) p.out_status[q] = (unsigned char)status;
    }
}

int launch_refine_relative_pose(const float* pixels, const float* conf, const float* weight, const double* cams_dev, const double* dist_dev,
                                int B, int V, int J, const int* pairs, int P, const double* rotation, const double* direction, double huber,
                                int max_iterations, double step_tolerance, double baseline, double* out_rotation, double* out_direction,
                                double* out_cams, double* out_error, double* out_cost0, double* out_cost, int* out_used, int* out_iterations,
                                unsigned char* out_status, hipStream_t s) {
    if (!pixels || !cams_dev || !pairs || !rotation || !direction || !out_rotation || !out_direction || !out_cams || !out_error)
        return MPL_E_INVALID;
    if (B <= 0 || V <= 0 || J <= 0 || P <= 0 || V > MPL_MAX_VIEWS || P > MPL_MAX_VIEWS || J > 64 || (long long)B * V * J > (1ll << 30) ||
        (long long)B * P * J > (1ll << 30))
        return MPL_E_INVALID;
    for (int q = 0; q < P; ++q) {
        const int a = pairs[2 * q], b = pairs[2 * q + 1];
        if (a < 0 || a >= V || b < 0 || b >= V || a == b) return MPL_E_INVALID;
    }
    if (max_iterations < 0 || max_iterations > 1000 || !(step_tolerance >= 0.0) || !(step_tolerance <= FINITE_MAX) || !(baseline > 0.0) ||
        !(baseline <= FINITE_MAX))
        return MPL_E_UNSUPPORTED;
    RefineRelativeParams p;
    p.px = pixels; p.conf = conf; p.weight = weight; p.cams = cams_dev; p.dist = dist_dev; p.rotation = rotation; p.direction = direction;
    p.out_rotation = out_rotation; p.out_direction = out_direction; p.out_cams = out_cams; p.out_error = out_error;
    p.out_cost0 = out_cost0; p.out_cost = out_cost; p.out_used = out_used; p.out_iterations = out_iterations; p.out_status = out_status;
    p.huber = huber > 0.0 ? huber : 0.0;
    p.tol = step_tolerance;
    p.baseline = baseline;
    p.N = (unsigned)(B * J); p.V = (unsigned)V; p.J = (unsigned)J; p.P = (unsigned)P; p.max_it = max_iterations;
    for (int q = 0; q < MPL_MAX_VIEWS; ++q) {
        p.va[q] = (unsigned char)(q < P ? pairs[2 * q] : 0);
        p.vb[q] = (unsigned char)(q < P ? pairs[2 * q + 1] : 0);
    }
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dist_dev) hipLaunchKernelGGL(refine_relative_kernel<true>, dim3((unsigned)P), dim3(RREL_THREADS), 0, s, p);
    else hipLaunchKernelGGL(refine_relative_kernel<false>, dim3((unsigned)P), dim3(RREL_THREADS), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
