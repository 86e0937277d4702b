// Locating cameras from scratch (mpl_locate_cameras): robust resection of every view from known 3D points and their detections.
//
// refine_cameras.hip starts from a pose that is nearly right; this file finds one where there is none, in the presence of wrong
// detections, by hypothesise-and-score.  Per view: H hypotheses, each the 6-point DLT of six observations drawn with the counter-based
// numbers of detrng.hpp, each scored over all observations of the view by the reprojection error in pixels, lens included, against a
// threshold; the winner has the most inliers, then the lowest truncated cost, then the lowest number.  The reference has no such
// step.  include/mpl_hip.h states the six steps; tests/locate_cameras_cases.py restates them in numpy.
//
// Three launches, all float64 on the float32 inputs:
//   1. locate_prepare_kernel, one workgroup per view: which observations take part, their undistorted normalised coordinates and a
//      compact record (point, pixel, weight; weight 0 = takes no part) into the workspace; centroid and scale of the participating
//      points, summed in a fixed order.
//   2. locate_hypotheses_kernel, one lane per hypothesis, one wave per workgroup.  The 12 x 12 system of a lane and the 12 x 12
//      rotations of its one-sided Jacobi (Hestenes) are 288 doubles, indexed by the loop counters of the sweep: as a per-lane array
//      they would live in scratch, so they live in LDS, lane-interleaved (element e of lane l at double e * 64 + l: 64 lanes read 512
//      contiguous bytes, no bank conflict), 144 KiB per wave.  Only the two columns of a rotation are in registers, every index a
//      constant.  The Jacobi works on A itself, not on A^T A: the null vector keeps the accuracy of its own singular value gap.  The
//      scoring loop stages the records 64 at a time in LDS; every lane reads the same address, a broadcast.  A lane sums its cost
//      over the observations in their order, so the bits do not depend on how the hypotheses are dealt to workgroups.
//   3. locate_select_kernel, one workgroup per view: the lexicographic winner (a total order, so any reduction tree gives the same
//      one), the record, the inlier mask, the count and the error of the winner.
// No atomics, nothing read back, no synchronisation.  The scaffold of the three launches is consensus.hpp, shared with
// relative_pose.hip; the rotation of the Jacobi, the 3 x 3 factorisation and the LDS addressing are hestenes.hpp.
#include "common.hpp"
#include "consensus.hpp"
#include "hestenes.hpp"
#include "reprojection.hpp"

namespace mpl {

namespace {

using consensus::LANES;
using consensus::THREADS;
using consensus::WAVES;

constexpr int LCAM_SAMPLE = 6;
constexpr int LCAM_REC = 6;              // a record, floats: X0 X1 X2 q0 q1 w; w = 0: takes no part
constexpr int LCAM_ROWS = 24;            // a column of the stacked [A; V]: 12 rows of the system over 12 of the rotations
constexpr int LCAM_SYSTEM = LCAM_ROWS * 12;
constexpr int LCAM_SWEEPS = 30;          // a cap: the samples of the tests are orthogonal to LCAM_ROT_EPS after 6 to 9
constexpr double LCAM_ROT_EPS = 1e-15;   // columns with |a . b| <= this * |a| |b| are not turned
constexpr int LCAM_LDS = LCAM_SYSTEM * LANES * 8 + consensus::TILE * LCAM_REC * 4;

// The workspace of a view, in doubles: a header | y (N,2) | the records (N,LCAM_REC) as floats
enum { LCAM_M = 0, LCAM_S = 3, LCAM_COUNT = 4, LCAM_USABLE = 5, LCAM_HDR = 8 };

struct LocateParams {
    const float* points;      // (B,J,3)
    const float* px;          // (B,V,J,2)
    const float* conf;        // (B,V,J) or null
    const double* cams;       // device (V,16)
    const double* dist;       // device (V,5) or null
    double* ws;
    double* out_cams;         // (V,16); may be cams
    float* out_inliers;       // (B,V,J)
    int* out_count;           // (V)
    int* out_best;            // (V)
    double* out_error;        // (V)
    unsigned char* out_status;   // (V)
    double* poses;            // (V,H,12)
    double* scores;           // (V,H,2)
    double tau2;
    unsigned N, V, J, H, fixed_mask;          // N = B J observations per view; B V J <= 2^30
    unsigned long long keys[MPL_MAX_VIEWS];
};

__device__ __forceinline__ double* lcam_header(const LocateParams& p, unsigned v) { return p.ws + (size_t)v * (LCAM_HDR + 5 * (size_t)p.N); }
__device__ __forceinline__ double* lcam_y(const LocateParams& p, unsigned v) { return lcam_header(p, v) + LCAM_HDR; }
__device__ __forceinline__ float* lcam_records(const LocateParams& p, unsigned v) {
    return reinterpret_cast<float*>(lcam_header(p, v) + LCAM_HDR + 2 * (size_t)p.N);
}

// |r|^2 of the observation of record r under the camera record c, and whether the point is in front: the projection of
// refine_cameras.hip.  One statement for the scoring loop and the winner's mask, so that both count the same observations
__device__ __forceinline__ double lcam_residual2(const double (&c)[16], const Distortion d, const float* r, bool& front) {
    const Camera cam{c};
    double xc, yc, zc;
    camera_coords(c, (double)r[0], (double)r[1], (double)r[2], xc, yc, zc);
    front = zc > CAMERA_Z_MIN;
    const Normalized yd = distort_normalized(xc / zc, yc / zc, d);
    const Pixel px = pixel_of(cam, yd.x, yd.y);
    const double r0 = px.x - (double)r[3], r1 = px.y - (double)r[4];
    return r0 * r0 + r1 * r1;
}

}  // namespace

// ---- 1. participation, normalised observations, records, centroid and scale
template <bool LENS>
__global__ __launch_bounds__(THREADS) void locate_prepare_kernel(const LocateParams p) {
    __shared__ double sh_cam[21], sh_part[WAVES][4], sh_tot[4];
    const unsigned v = blockIdx.x, tid = threadIdx.x;
    if (tid < 16) sh_cam[tid] = p.cams[(size_t)v * 16 + tid];
    else if (LENS && tid < 21) sh_cam[tid] = p.dist[(size_t)v * 5 + (tid - 16)];
    __syncthreads();
    double c[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = sh_cam[k];
    const Distortion d = distortion_from<LENS>(sh_cam + 16);
    const Camera cam{c};
    bool finite = true;                                  // of the record, only the intrinsics are read
#pragma unroll
    for (int k = 0; k < 4; ++k) finite = finite && fabs(c[k]) <= FINITE_MAX;
    double* yv = lcam_y(p, v);
    float* rec = lcam_records(p, v);

    double a[4] = {0.0, 0.0, 0.0, 0.0};                  // sum X, and the count
    for (unsigned i = tid; i < p.N; i += THREADS) {
        const unsigned b = i / p.J, j = i - b * p.J;
        const unsigned o = (b * p.V + v) * p.J + j;            // below 2^30, so twice it fits 32 bits
        const double w = p.conf ? (double)p.conf[o] : 1.0;
        const float q0 = p.px[o * 2u], q1 = p.px[o * 2u + 1u];
        const float* x = p.points + (size_t)i * 3;
        const float x0 = x[0], x1 = x[1], x2 = x[2];
        // takes part: a finite weight > 0, a finite pixel, a finite point -- and a pixel that goes back through the lens
        bool part = finite && takes_part(w) && isfinite(q0) && isfinite(q1) && isfinite(x0) && isfinite(x1) && isfinite(x2);
        double y0 = 0.0, y1 = 0.0;
        if (part) {
            double xu, yu;
            part = undistort_pixel(c, d, (double)q0, (double)q1, xu, yu);
            y0 = (xu - cam.cx()) / cam.fx();
            y1 = (yu - cam.cy()) / cam.fy();
        }
        yv[2 * (size_t)i] = y0;
        yv[2 * (size_t)i + 1] = y1;
        float* r = rec + LCAM_REC * (size_t)i;
        r[0] = x0; r[1] = x1; r[2] = x2; r[3] = q0; r[4] = q1;
        r[5] = part ? (float)w : 0.0f;                   // a float32 confidence or 1: exact
        if (part) {
            a[0] += (double)x0; a[1] += (double)x1; a[2] += (double)x2; a[3] += 1.0;
        }
    }
    consensus::block_sum(a, sh_part, sh_tot);
    const double count = a[3], m0 = a[0] / count, m1 = a[1] / count, m2 = a[2] / count;
    double q[1] = {0.0};
    for (unsigned i = tid; i < p.N; i += THREADS) {       // the records this thread wrote itself
        const float* r = rec + LCAM_REC * (size_t)i;
        if (!(r[5] > 0.0f)) continue;
        const double d0 = (double)r[0] - m0, d1 = (double)r[1] - m1, d2 = (double)r[2] - m2;
        q[0] += d0 * d0 + d1 * d1 + d2 * d2;
    }
    consensus::block_sum(q, sh_part, sh_tot);
    if (tid == 0) {
        double* hdr = lcam_header(p, v);
        hdr[LCAM_M] = m0; hdr[LCAM_M + 1] = m1; hdr[LCAM_M + 2] = m2;
        hdr[LCAM_S] = 1.0 / sqrt(q[0] / count / 3.0);
        hdr[LCAM_COUNT] = count;
        hdr[LCAM_USABLE] = (finite && count >= (double)LCAM_SAMPLE) ? 1.0 : 0.0;
        hdr[6] = 0.0; hdr[7] = 0.0;
    }
}

// ---- 2. one lane per hypothesis: sample, solve, score
template <bool LENS>
__global__ __launch_bounds__(LANES) void locate_hypotheses_kernel(const LocateParams p) {
    extern __shared__ __attribute__((aligned(16))) double lcam_lds[];
    const Strided<LANES> sys{lcam_lds + threadIdx.x};    // element (row r, column c) of this lane at sys[c * LCAM_ROWS + r]
    float* tile = reinterpret_cast<float*>(lcam_lds + LCAM_SYSTEM * LANES);
    __shared__ double sh_cam[21], sh_hdr[LCAM_HDR];
    const unsigned lane = threadIdx.x, v = blockIdx.y, h = blockIdx.x * LANES + lane;
    if (lane < 16) sh_cam[lane] = p.cams[(size_t)v * 16 + lane];
    else if (LENS && lane < 21) sh_cam[lane] = p.dist[(size_t)v * 5 + (lane - 16)];
    else if (lane >= 32 && lane < 32 + LCAM_HDR) sh_hdr[lane - 32] = lcam_header(p, v)[lane - 32];
    __syncthreads();
    const consensus::Hypothesis hyp = consensus::hypothesis_at(p.poses, p.scores, v, p.H, h);
    // a view that is passed through, or that has no six observations: every hypothesis is void (the same for the whole workgroup)
    if ((p.fixed_mask >> v & 1u) || sh_hdr[LCAM_USABLE] == 0.0) {
        hyp.write_void();
        return;
    }
    double c[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = sh_cam[k];
    const Distortion d = distortion_from<LENS>(sh_cam + 16);
    const double m0 = sh_hdr[LCAM_M], m1 = sh_hdr[LCAM_M + 1], m2 = sh_hdr[LCAM_M + 2], s = sh_hdr[LCAM_S];
    const double* yv = lcam_y(p, v);
    const float* rec = lcam_records(p, v);

    unsigned pick[LCAM_SAMPLE];
    bool ok = consensus::draw_distinct(p.keys[v], h, p.N, [rec](unsigned n) { return rec[LCAM_REC * (size_t)n + 5] > 0.0f; }, pick);

    // the system [Xh, 0, -y0 Xh; 0, Xh, -y1 Xh] on Xh = (s (X - m), 1), over the identity that collects the rotations
    double X[LCAM_SAMPLE][3];                            // the sample points as given: the depth test at the end reads them
    double xh[LCAM_SAMPLE][3];
#pragma unroll
    for (int i = 0; i < LCAM_SAMPLE; ++i) {
        const float* r = rec + LCAM_REC * (size_t)pick[i];
        X[i][0] = (double)r[0]; X[i][1] = (double)r[1]; X[i][2] = (double)r[2];
        xh[i][0] = s * (X[i][0] - m0); xh[i][1] = s * (X[i][1] - m1); xh[i][2] = s * (X[i][2] - m2);
        const double y0 = yv[2 * (size_t)pick[i]], y1 = yv[2 * (size_t)pick[i] + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double e = k < 3 ? xh[i][k] : 1.0;
            sys[(k + 0) * LCAM_ROWS + 2 * i] = e;
            sys[(k + 4) * LCAM_ROWS + 2 * i] = 0.0;
            sys[(k + 8) * LCAM_ROWS + 2 * i] = -y0 * e;
            sys[(k + 0) * LCAM_ROWS + 2 * i + 1] = 0.0;
            sys[(k + 4) * LCAM_ROWS + 2 * i + 1] = e;
            sys[(k + 8) * LCAM_ROWS + 2 * i + 1] = -y1 * e;
        }
    }
    for (int col = 0; col < 12; ++col)
        for (int r = 0; r < 12; ++r) sys[col * LCAM_ROWS + 12 + r] = r == col ? 1.0 : 0.0;

    // one-sided Jacobi: rotations from the right make the columns of A orthogonal, A V = U S; cyclic sweeps until no lane of the
    // wave turns a pair (a value that is not a number turns none)
#pragma unroll 1
    for (int sweep = 0; sweep < LCAM_SWEEPS; ++sweep) {
        bool turned = false;
#pragma unroll 1
        for (int ca = 0; ca < 11; ++ca) {
#pragma unroll 1
            for (int cb = ca + 1; cb < 12; ++cb) {
                double a[LCAM_ROWS], b[LCAM_ROWS];
#pragma unroll
                for (int r = 0; r < LCAM_ROWS; ++r) {
                    a[r] = sys[ca * LCAM_ROWS + r];
                    b[r] = sys[cb * LCAM_ROWS + r];
                }
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 12; ++r) {
                    alpha += a[r] * a[r];
                    beta += b[r] * b[r];
                    gamma += a[r] * b[r];
                }
                if (fabs(gamma) > LCAM_ROT_EPS * sqrt(alpha * beta)) {
                    const Rotation rot = hestenes_rotation<true>(alpha, beta, gamma);
                    const double cs = rot.cs, sn = rot.sn;
#pragma unroll
                    for (int r = 0; r < LCAM_ROWS; ++r) {
                        sys[ca * LCAM_ROWS + r] = cs * a[r] - sn * b[r];
                        sys[cb * LCAM_ROWS + r] = sn * a[r] + cs * b[r];
                    }
                    turned = true;
                }
            }
        }
        if (!__any(turned)) break;
    }
    // the null vector: the column of V under the shortest column of A V (the lowest column among equals)
    int kmin = 0;
    double smin = __builtin_inf();
    for (int col = 0; col < 12; ++col) {
        double n2 = 0.0;
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            const double e = sys[col * LCAM_ROWS + r];
            n2 += e * e;
        }
        if (n2 < smin) {
            smin = n2;
            kmin = col;
        }
    }
    double P[12];
#pragma unroll
    for (int r = 0; r < 12; ++r) P[r] = sys[kmin * LCAM_ROWS + 12 + r];
    // the sign that puts the six sample points in front, summed
    double depth = 0.0;
#pragma unroll
    for (int i = 0; i < LCAM_SAMPLE; ++i) depth += P[8] * xh[i][0] + P[9] * xh[i][1] + P[10] * xh[i][2] + P[11];
    if (depth < 0.0) {
#pragma unroll
        for (int r = 0; r < 12; ++r) P[r] = -P[r];
    }
    // M = U S W^T by the same Jacobi on 3 x 3: R = U W^T, the shortest column turned over where det M < 0
    double M[3][3] = {{P[0], P[1], P[2]}, {P[4], P[5], P[6]}, {P[8], P[9], P[10]}};
    double W[3][3], sv[3], sg[3];
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    const int last = factor3(M, W, sv);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ok = ok && sv[k] > 0.0;
        sg[k] = ((det < 0.0 && k == last) ? -1.0 : 1.0) / sv[k];
    }
    const double scale = (sv[0] + sv[1] + sv[2]) / 3.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[4 + 3 * i + k] = sg[0] * M[i][0] * W[k][0] + sg[1] * M[i][1] * W[k][1] + sg[2] * M[i][2] * W[k][2];
    }
    // x_cam ~ R s (X - m) + t with t = p4 / scale: the centre is m - R^T t / s
    const double t0 = P[3] / scale, t1 = P[7] / scale, t2 = P[11] / scale;
    c[13] = m0 - (c[4] * t0 + c[7] * t1 + c[10] * t2) / s;
    c[14] = m1 - (c[5] * t0 + c[8] * t1 + c[11] * t2) / s;
    c[15] = m2 - (c[6] * t0 + c[9] * t1 + c[12] * t2) / s;
#pragma unroll
    for (int k = 4; k < 16; ++k) ok = ok && fabs(c[k]) <= FINITE_MAX;
#pragma unroll
    for (int i = 0; i < LCAM_SAMPLE; ++i) {
        double xc, yc, zc;
        camera_coords(c, X[i][0], X[i][1], X[i][2], xc, yc, zc);
        ok = ok && zc > CAMERA_Z_MIN;
    }
    if (hyp.live) {
#pragma unroll
        for (int k = 0; k < 12; ++k) hyp.pose[k] = ok ? c[4 + k] : __builtin_nan("");
    }

    // the score over all observations in their order; a void lane goes along and is overwritten at the end
    const consensus::Score sc = consensus::score_tiled<float, LCAM_REC, float2>(
        rec, p.N, tile, p.tau2, [&c, d](const float* r, bool& front) { return lcam_residual2(c, d, r, front); });
    hyp.write_score(ok, sc.count, sc.cost);
}

// ---- 3. the winner of a view, its record, mask, count and error
template <bool LENS>
__global__ __launch_bounds__(THREADS) void locate_select_kernel(const LocateParams p) {
    __shared__ double sh_cam[21], sh_part[WAVES][4], sh_tot[4], sh_usable;
    const unsigned v = blockIdx.x, tid = threadIdx.x;
    // the given record, read before its row of out_cams is written (out_cams may be cams)
    if (tid < 16) sh_cam[tid] = p.cams[(size_t)v * 16 + tid];
    else if (LENS && tid < 21) sh_cam[tid] = p.dist[(size_t)v * 5 + (tid - 16)];
    else if (tid == 32) sh_usable = lcam_header(p, v)[LCAM_USABLE];
    __syncthreads();
    const bool fixed = p.fixed_mask >> v & 1u;
    const consensus::Winner best = consensus::select_winner(p.scores, v, p.H, !fixed && sh_usable != 0.0);
    const bool located = best.located();

    // the record that is scored: the winner's pose, or the given one of a view that is passed through
    double c[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = sh_cam[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[4 + k] = located ? p.poses[((size_t)v * p.H + (unsigned)best.h) * 12 + k] : sh_cam[4 + k];
    const Distortion d = distortion_from<LENS>(sh_cam + 16);
    const float* rec = lcam_records(p, v);
    const bool scored = located || fixed;
    double a[2] = {0.0, 0.0};                            // sum |r|^2 over the inliers, and their count
    for (unsigned i = tid; i < p.N; i += THREADS) {
        const unsigned b = i / p.J, j = i - b * p.J;
        const unsigned o = (b * p.V + v) * p.J + j;
        const float* r = rec + LCAM_REC * (size_t)i;
        bool in = false;
        if (scored && r[5] > 0.0f) {
            bool front;
            const double r2 = lcam_residual2(c, d, r, front);
            in = front && r2 <= p.tau2;
            if (in) {
                a[0] += r2;
                a[1] += 1.0;
            }
        }
        p.out_inliers[o] = in ? 1.0f : 0.0f;
    }
    consensus::block_sum(a, sh_part, sh_tot);
    if (tid == 0) {
        double* row = p.out_cams + (size_t)v * 16;
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = c[k];      // the given bits where nothing was located
        p.out_count[v] = (int)a[1];
        p.out_best[v] = fixed ? -1 : best.h;
        p.out_error[v] = a[1] > 0.0 ? sqrt(a[0] / a[1]) : __builtin_nan("");
        p.out_status[v] = (unsigned char)(fixed ? LM_PASSED_THROUGH : located ? LM_CONVERGED : LM_INVALID);
    }
}

size_t locate_cameras_workspace_bytes(int B, int V, int J) {
    if (!consensus::sizes_ok(B, V, J)) return 0;
    return (size_t)V * (LCAM_HDR + 5 * (size_t)B * (size_t)J) * sizeof(double);
}

int launch_locate_cameras(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                          int B, int V, int J, double threshold, int hypotheses, const unsigned long long* keys, unsigned fixed_mask,
                          void* workspace, size_t workspace_bytes, double* out_cams, float* out_inliers, int* out_count, int* out_best,
                          double* out_error, unsigned char* out_status, double* out_poses, double* out_scores, hipStream_t s) {
    if (const int e = refine_args_check(points, pixels, cams_dev, out_cams, out_error, B, V, J, 0, 0.0)) return e;
    if (!keys || !out_inliers || !out_count || !out_best || !out_status || !out_poses || !out_scores) return MPL_E_INVALID;
    if (const int e = consensus::options_check(threshold, hypotheses)) return e;
    if (!workspace || workspace_bytes < locate_cameras_workspace_bytes(B, V, J)) return MPL_E_WORKSPACE;
    LocateParams p;
    p.points = points; p.px = pixels; p.conf = conf; p.cams = cams_dev; p.dist = dist_dev;
    p.ws = static_cast<double*>(workspace);
    p.out_cams = out_cams; p.out_inliers = out_inliers; p.out_count = out_count; p.out_best = out_best; p.out_error = out_error;
    p.out_status = out_status; p.poses = out_poses; p.scores = out_scores;
    p.tau2 = threshold * threshold;
    p.N = (unsigned)(B * J); p.V = (unsigned)V; p.J = (unsigned)J; p.H = (unsigned)hypotheses; p.fixed_mask = fixed_mask;
    for (int v = 0; v < MPL_MAX_VIEWS; ++v) p.keys[v] = v < V ? keys[v] : 0ull;
    return consensus::launch<locate_prepare_kernel<true>, locate_prepare_kernel<false>, locate_hypotheses_kernel<true>,
                             locate_hypotheses_kernel<false>, locate_select_kernel<true>, locate_select_kernel<false>>(
        dist_dev != nullptr, p.V, p.H, LCAM_LDS, p, s);
}

}  // namespace mpl
