// Relative pose of two views from their detections alone (mpl_relative_pose): robust five-point solver.
//
// locate_cameras.hip needs 3D points; this file is the step before it, for a rig of which nothing is known but the intrinsics.  Per
// pair of views (a, b): H hypotheses, each the at most ten essential matrices through five correspondences drawn with the
// counter-based numbers of detrng.hpp (five_point.hpp), each candidate scored over all correspondences of the pair by the signed
// Sampson distance in pixels against a threshold; a hypothesis keeps its best candidate, and the winner has the most inliers, then
// the lowest truncated cost, then the lowest number.  The reference has no such step.  include/mpl_hip.h states the five steps;
// tests/relative_pose_cases.py restates them in numpy.
//
// Three launches on the scaffold of consensus.hpp, which locate_cameras.hip shares, all float64 on the float32 inputs:
//   1. relative_prepare_kernel, one workgroup per pair: which slots take part, their undistorted pixels, normalised coordinates and
//      weight into the workspace; their count, summed in a fixed order.
//   2. relative_hypotheses_kernel, one lane per hypothesis, one wave per workgroup.  What the solver indexes by a loop counter -- the
//      14 x 9 system of the Jacobi, the 10 x 20 elimination, the Sturm chain, the roots -- is 249 doubles a lane and lives in LDS,
//      lane-interleaved (Strided of hestenes.hpp; 125 KiB per wave), not in scratch.  The candidates are scored one after the other,
//      the records staged 64 at a time in LDS; a lane sums its cost over the slots in their order, so the bits do not depend on how
//      the hypotheses are dealt to workgroups.
//   3. relative_select_kernel, one workgroup per pair: the lexicographic winner, its pose, records, inlier mask, count and error.
// No atomics, nothing read back, no synchronisation.
#include "common.hpp"
#include "consensus.hpp"
#include "five_point.hpp"
#include "reprojection.hpp"

namespace mpl {

namespace {

using consensus::LANES;
using consensus::THREADS;
using consensus::WAVES;

constexpr int RPOSE_REC = 5;             // a record, doubles: u_a (2), u_b (2), w; w = 0: takes no part
constexpr int RPOSE_LDS = (fivept::FP_DOUBLES * LANES + consensus::TILE * RPOSE_REC) * 8;

// The workspace of a pair, in doubles: a header | the records (N,5) | y_a, y_b (N,4)
enum { RPOSE_COUNT = 0, RPOSE_USABLE = 1, RPOSE_HDR = 8 };

struct RelativeParams {
    const float* px;          // (B,V,J,2)
    const float* conf;        // (B,V,J) or null
    const double* cams;       // device (V,16)
    const double* dist;       // device (V,5) or null
    double* ws;
    double* out_rotation;     // (P,9)
    double* out_direction;    // (P,3)
    double* out_cams;         // (P,2,16)
    float* out_inliers;       // (B,P,J)
    int* out_count;           // (P)
    int* out_best;            // (P)
    double* out_error;        // (P)
    unsigned char* out_status;   // (P)
    double* poses;            // (P,H,12)
    double* scores;           // (P,H,2)
    int* roots;               // (P,H)
    double tau2, baseline;
    unsigned N, V, J, P, H;                   // N = B J slots per pair; B V J <= 2^30
    unsigned char va[MPL_MAX_VIEWS], vb[MPL_MAX_VIEWS];
    unsigned long long keys[MPL_MAX_VIEWS];
};

__device__ __forceinline__ double* rpose_header(const RelativeParams& p, unsigned q) { return p.ws + (size_t)q * (RPOSE_HDR + 9 * (size_t)p.N); }
__device__ __forceinline__ double* rpose_records(const RelativeParams& p, unsigned q) { return rpose_header(p, q) + RPOSE_HDR; }
__device__ __forceinline__ double* rpose_y(const RelativeParams& p, unsigned q) { return rpose_records(p, q) + RPOSE_REC * (size_t)p.N; }

// F = K_b^-T [t]x R K_a^-1 of a pose (R row-major, then t); ka, kb: fx fy cx cy of the two views
__device__ __forceinline__ void rpose_fundamental(const double (&pose)[12], const double* ka, const double* kb, double (&F)[9]) {
    const double t0 = pose[9], t1 = pose[10], t2 = pose[11];
    double E[3][3], M[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        E[0][c] = t1 * pose[6 + c] - t2 * pose[3 + c];
        E[1][c] = t2 * pose[c] - t0 * pose[6 + c];
        E[2][c] = t0 * pose[3 + c] - t1 * pose[c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[r][0] = E[r][0] / ka[0];
        M[r][1] = E[r][1] / ka[1];
        M[r][2] = E[r][2] - E[r][0] * (ka[2] / ka[0]) - E[r][1] * (ka[3] / ka[1]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F[c] = M[0][c] / kb[0];
        F[3 + c] = M[1][c] / kb[1];
        F[6 + c] = M[2][c] - (kb[2] / kb[0]) * M[0][c] - (kb[3] / kb[1]) * M[1][c];
    }
}

// d^2 of one slot, d the signed Sampson distance in pixels: u_b^T F u_a over the root of the four squared gradient entries.  One
// statement for the scoring loop and the winner's mask, so that both count the same slots
__device__ __forceinline__ double rpose_sampson2(const double (&F)[9], double a0, double a1, double b0, double b1) {
    const double fa0 = F[0] * a0 + F[1] * a1 + F[2], fa1 = F[3] * a0 + F[4] * a1 + F[5], fa2 = F[6] * a0 + F[7] * a1 + F[8];
    const double fb0 = F[0] * b0 + F[3] * b1 + F[6], fb1 = F[1] * b0 + F[4] * b1 + F[7];
    const double num = b0 * fa0 + b1 * fa1 + fa2;
    return (num * num) / (fa0 * fa0 + fa1 * fa1 + fb0 * fb0 + fb1 * fb1);
}

// s ((a0 b0 + a1 b1) + a2 b2) with every product and sum rounded on its own: no contraction into multiply-adds
__device__ __forceinline__ double rpose_scaled_dot3(double s, double a0, double b0, double a1, double b1, double a2, double b2) {
#pragma clang fp contract(off)
    const double d = (a0 * b0 + a1 * b1) + a2 * b2;
    return s * d;
}

}  // namespace

// ---- 1. participation, undistorted pixels, normalised coordinates, weights and their count
template <bool LENS>
__global__ __launch_bounds__(THREADS) void relative_prepare_kernel(const RelativeParams p) {
    __shared__ double sh_cam[2][21], sh_part[WAVES][2], sh_tot[2];
    const unsigned q = blockIdx.x, tid = threadIdx.x;
    const unsigned va = p.va[q], vb = p.vb[q];
    if (tid < 64) {
        const unsigned side = tid >> 5, k = tid & 31u, v = side ? vb : va;
        if (k < 16) sh_cam[side][k] = p.cams[(size_t)v * 16 + k];
        else if (LENS && k < 21) sh_cam[side][k] = p.dist[(size_t)v * 5 + (k - 16)];
    }
    __syncthreads();
    double ca[16], cb[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        ca[k] = sh_cam[0][k];
        cb[k] = sh_cam[1][k];
    }
    const Distortion da = distortion_from<LENS>(sh_cam[0] + 16), db = distortion_from<LENS>(sh_cam[1] + 16);
    bool finite = true;                                  // of the records, only the intrinsics are read
#pragma unroll
    for (int k = 0; k < 4; ++k) finite = finite && fabs(ca[k]) <= FINITE_MAX && fabs(cb[k]) <= FINITE_MAX;
    double* rec = rpose_records(p, q);
    double* yv = rpose_y(p, q);

    double a[1] = {0.0};
    for (unsigned i = tid; i < p.N; i += THREADS) {
        const unsigned b = i / p.J, j = i - b * p.J;
        const unsigned oa = (b * p.V + va) * p.J + j, ob = (b * p.V + vb) * p.J + j;      // below 2^30, so twice it fits 32 bits
        const double wa = p.conf ? (double)p.conf[oa] : 1.0, wb = p.conf ? (double)p.conf[ob] : 1.0;
        const float qa0 = p.px[oa * 2u], qa1 = p.px[oa * 2u + 1u], qb0 = p.px[ob * 2u], qb1 = p.px[ob * 2u + 1u];
        // takes part: in both views a finite weight > 0 and a finite pixel that goes back through the lens
        bool part = finite && takes_part(wa) && takes_part(wb) && isfinite(qa0) && isfinite(qa1) && isfinite(qb0) && isfinite(qb1);
        double ua0 = 0.0, ua1 = 0.0, ub0 = 0.0, ub1 = 0.0;
        if (part) {
            part = undistort_pixel(ca, da, (double)qa0, (double)qa1, ua0, ua1);
            part = undistort_pixel(cb, db, (double)qb0, (double)qb1, ub0, ub1) && part;
        }
        double* r = rec + RPOSE_REC * (size_t)i;
        double* y = yv + 4 * (size_t)i;
        r[0] = part ? ua0 : 0.0; r[1] = part ? ua1 : 0.0; r[2] = part ? ub0 : 0.0; r[3] = part ? ub1 : 0.0;
        r[4] = part ? wa * wb : 0.0;
        y[0] = part ? (ua0 - ca[2]) / ca[0] : 0.0;
        y[1] = part ? (ua1 - ca[3]) / ca[1] : 0.0;
        y[2] = part ? (ub0 - cb[2]) / cb[0] : 0.0;
        y[3] = part ? (ub1 - cb[3]) / cb[1] : 0.0;
        if (part) a[0] += 1.0;
    }
    consensus::block_sum(a, sh_part, sh_tot);
    if (tid == 0) {
        double* hdr = rpose_header(p, q);
        hdr[RPOSE_COUNT] = a[0];
        hdr[RPOSE_USABLE] = (finite && a[0] >= (double)fivept::FP_SAMPLE) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 2; k < RPOSE_HDR; ++k) hdr[k] = 0.0;
    }
}

// ---- 2. one lane per hypothesis: sample, solve, score every candidate
__global__ __launch_bounds__(LANES) void relative_hypotheses_kernel(const RelativeParams p) {
    extern __shared__ __attribute__((aligned(16))) double rpose_lds[];
    const Strided<LANES> mem{rpose_lds + threadIdx.x};
    double* tile = rpose_lds + fivept::FP_DOUBLES * LANES;
    __shared__ double sh_k[8], sh_hdr[RPOSE_HDR];
    const unsigned lane = threadIdx.x, q = blockIdx.y, h = blockIdx.x * LANES + lane;
    if (lane < 4) sh_k[lane] = p.cams[(size_t)p.va[q] * 16 + lane];
    else if (lane < 8) sh_k[lane] = p.cams[(size_t)p.vb[q] * 16 + (lane - 4)];
    else if (lane >= 32 && lane < 32 + RPOSE_HDR) sh_hdr[lane - 32] = rpose_header(p, q)[lane - 32];
    __syncthreads();
    const consensus::Hypothesis hyp = consensus::hypothesis_at(p.poses, p.scores, q, p.H, h);
    // a pair that has no five correspondences: every hypothesis is void (the same for the whole workgroup)
    if (sh_hdr[RPOSE_USABLE] == 0.0) {
        hyp.write_void();
        if (hyp.live) p.roots[(size_t)q * p.H + h] = 0;
        return;
    }
    const double* rec = rpose_records(p, q);
    const double* yv = rpose_y(p, q);

    unsigned pick[fivept::FP_SAMPLE];
    const bool ok = consensus::draw_distinct(p.keys[q], h, p.N, [rec](unsigned n) { return rec[RPOSE_REC * (size_t)n + 4] > 0.0; }, pick);
    double ya[fivept::FP_SAMPLE][2], yb[fivept::FP_SAMPLE][2];
#pragma unroll
    for (int i = 0; i < fivept::FP_SAMPLE; ++i) {
        const double* y = yv + 4 * (size_t)pick[i];
        ya[i][0] = y[0]; ya[i][1] = y[1]; yb[i][0] = y[2]; yb[i][1] = y[3];
    }

    // A lane whose draw failed solves on whatever its slots hold and is set aside afterwards: its wave mates need the same
    // instructions anyway, every loop of the solver has a fixed bound, and a value that is not a number ends the Jacobi (nothing
    // is turned), the elimination (no pivot) and the chain (degree -1) early; nothing of it is written
    double basis[4][9], Bz[3][13];
    int n_roots = fivept::solve(mem, ya, yb, basis, Bz);
    if (!ok) n_roots = 0;

    // every candidate scored over all slots in their order; the best one kept: most inliers, then the lowest cost, then the first
    double best_pose[12], best_cost = __builtin_inf();
    int best_count = -1;
#pragma unroll
    for (int k = 0; k < 12; ++k) best_pose[k] = __builtin_nan("");
#pragma unroll 1
    for (int cand = 0; cand < fivept::FP_MAX_ROOTS; ++cand) {
        if (!__any(cand < n_roots)) break;                           // the same for the whole wave: the barriers below are reached by all
        const bool mine = cand < n_roots;
        const double z = mem[fivept::FP_ROOTS_AT + cand];
        double E[9], pose[12], F[9];
        double sa[fivept::FP_SAMPLE][2], sb[fivept::FP_SAMPLE][2];   // the samples, read again: ten fewer registers held across the solver
#pragma unroll
        for (int i = 0; i < fivept::FP_SAMPLE; ++i) {
            const double* y = yv + 4 * (size_t)pick[i];
            sa[i][0] = y[0]; sa[i][1] = y[1]; sb[i][0] = y[2]; sb[i][1] = y[3];
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = 0.0;
        const bool valid = mine && fivept::essential_at(mem, basis, Bz, z, E) && fivept::pose_of(E, sa, sb, pose);
        rpose_fundamental(pose, sh_k, sh_k + 4, F);
        const auto sampson2 = [&F](const double* r, bool& counts) {
            counts = true;                               // a slot behind a camera has a distance like any other
            return rpose_sampson2(F, r[0], r[1], r[2], r[3]);
        };
        const consensus::Score sc = consensus::score_tiled<double, RPOSE_REC, double>(rec, p.N, tile, p.tau2, sampson2);
        if (valid && (sc.count > best_count || (sc.count == best_count && sc.cost < best_cost))) {
            best_count = sc.count;
            best_cost = sc.cost;
#pragma unroll
            for (int k = 0; k < 12; ++k) best_pose[k] = pose[k];
        }
    }
    if (hyp.live) {
#pragma unroll
        for (int k = 0; k < 12; ++k) hyp.pose[k] = best_pose[k];
        p.roots[(size_t)q * p.H + h] = n_roots;
    }
    hyp.write_score(best_count >= 0, best_count, best_cost);
}

// ---- 3. the winner of a pair, its pose, records, mask, count and error
__global__ __launch_bounds__(THREADS) void relative_select_kernel(const RelativeParams p) {
    __shared__ double sh_k[8], sh_part[WAVES][2], sh_tot[2], sh_usable;
    const unsigned q = blockIdx.x, tid = threadIdx.x;
    if (tid < 4) sh_k[tid] = p.cams[(size_t)p.va[q] * 16 + tid];
    else if (tid < 8) sh_k[tid] = p.cams[(size_t)p.vb[q] * 16 + (tid - 4)];
    else if (tid == 32) sh_usable = rpose_header(p, q)[RPOSE_USABLE];
    __syncthreads();
    const consensus::Winner best = consensus::select_winner(p.scores, q, p.H, sh_usable != 0.0);
    const bool located = best.located();

    double pose[12], F[9];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = located ? p.poses[((size_t)q * p.H + (unsigned)best.h) * 12 + k] : 0.0;
    rpose_fundamental(pose, sh_k, sh_k + 4, F);
    const double* rec = rpose_records(p, q);
    double a[2] = {0.0, 0.0};                            // sum d^2 over the inliers, and their count
    for (unsigned i = tid; i < p.N; i += THREADS) {
        const unsigned b = i / p.J, j = i - b * p.J;
        const double* r = rec + RPOSE_REC * (size_t)i;
        bool in = false;
        if (located && r[4] > 0.0) {
            const double d2 = rpose_sampson2(F, r[0], r[1], r[2], r[3]);
            in = d2 <= p.tau2;
            if (in) {
                a[0] += d2;
                a[1] += 1.0;
            }
        }
        p.out_inliers[((size_t)b * p.P + q) * p.J + j] = in ? 1.0f : 0.0f;
    }
    consensus::block_sum(a, sh_part, sh_tot);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        double* ra = p.out_cams + (size_t)q * 32;
        double* rb = ra + 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ra[k] = sh_k[k];
            rb[k] = sh_k[4 + k];
        }
        // view a is the gauge: R = I, centre 0; view b has R and the centre -baseline R^T t
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            ra[4 + k] = located ? ((k % 4 == 0) ? 1.0 : 0.0) : nan;
            rb[4 + k] = located ? pose[k] : nan;
            p.out_rotation[(size_t)q * 9 + k] = located ? pose[k] : nan;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ra[13 + k] = located ? 0.0 : nan;
            // every product and sum rounded on its own, in this order: the record is the same bits wherever it is formed
            rb[13 + k] = located ? -rpose_scaled_dot3(p.baseline, pose[k], pose[9], pose[3 + k], pose[10], pose[6 + k], pose[11]) : nan;
            p.out_direction[(size_t)q * 3 + k] = located ? pose[9 + k] : nan;
        }
        p.out_count[q] = (int)a[1];
        p.out_best[q] = best.h;
        p.out_error[q] = a[1] > 0.0 ? sqrt(a[0] / a[1]) : nan;
        p.out_status[q] = (unsigned char)(located ? LM_CONVERGED : LM_INVALID);
    }
}

size_t relative_pose_workspace_bytes(int B, int P, int J) {
    if (!consensus::sizes_ok(B, P, J)) return 0;
    return (size_t)P * (RPOSE_HDR + 9 * (size_t)B * (size_t)J) * sizeof(double);
}

int launch_relative_pose(const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev, int B, int V, int J,
                         const int* pairs, int P, double threshold, int hypotheses, const unsigned long long* keys, double baseline,
                         void* workspace, size_t workspace_bytes, double* out_rotation, double* out_direction, double* out_cams,
                         float* out_inliers, int* out_count, int* out_best, double* out_error, unsigned char* out_status, double* out_poses,
                         double* out_scores, int* out_roots, hipStream_t s) {
    if (!pixels || !cams_dev || !pairs || !keys || !out_rotation || !out_direction || !out_cams || !out_inliers || !out_count || !out_best ||
        !out_error || !out_status || !out_poses || !out_scores || !out_roots)
        return MPL_E_INVALID;
    if (!consensus::sizes_ok(B, V, J) || !consensus::sizes_ok(B, P, J)) return MPL_E_INVALID;
    for (int q = 0; q < P; ++q) {
        const int a = pairs[2 * q], b = pairs[2 * q + 1];
        if (a < 0 || a >= V || b < 0 || b >= V || a == b) return MPL_E_INVALID;
    }
    if (const int e = consensus::options_check(threshold, hypotheses)) return e;
    if (!(baseline > 0.0) || !(baseline <= FINITE_MAX)) return MPL_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < relative_pose_workspace_bytes(B, P, J)) return MPL_E_WORKSPACE;
    RelativeParams p;
    p.px = pixels; p.conf = conf; p.cams = cams_dev; p.dist = dist_dev;
    p.ws = static_cast<double*>(workspace);
    p.out_rotation = out_rotation; p.out_direction = out_direction; p.out_cams = out_cams; p.out_inliers = out_inliers;
    p.out_count = out_count; p.out_best = out_best; p.out_error = out_error; p.out_status = out_status;
    p.poses = out_poses; p.scores = out_scores; p.roots = out_roots;
    p.tau2 = threshold * threshold;
    p.baseline = baseline;
    p.N = (unsigned)(B * J); p.V = (unsigned)V; p.J = (unsigned)J; p.P = (unsigned)P; p.H = (unsigned)hypotheses;
    for (int q = 0; q < MPL_MAX_VIEWS; ++q) {
        p.va[q] = (unsigned char)(q < P ? pairs[2 * q] : 0);
        p.vb[q] = (unsigned char)(q < P ? pairs[2 * q + 1] : 0);
        p.keys[q] = q < P ? keys[q] : 0ull;
    }
    return consensus::launch<relative_prepare_kernel<true>, relative_prepare_kernel<false>, relative_hypotheses_kernel,
                             relative_hypotheses_kernel, relative_select_kernel, relative_select_kernel>(dist_dev != nullptr, p.P, p.H,
                                                                                                         RPOSE_LDS, p, s);
}

}  // namespace mpl
