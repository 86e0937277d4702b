// Temporal smoothing of pose tracks on the device (mpl_smooth_tracks; the cost, the stopping rule and the statuses are stated once,
// in include/mpl_hip.h).  Every (segment, joint) track is one symmetric positive definite pentadiagonal system
//     (W' + smoothness D^T D) X = W' Y
// of the segment's length with three right sides, solved once in the plain mode and once per reweighting under the Huber cost.
// The reference has no such step: its estimators and this project's work on one frame at a time.
//
// One wave per track, grid (segments, joints).  A track of more than MPL_SMOOTH_SINGLE_MAX frames is cut into blocks of
// L = max(MPL_SMOOTH_CHUNK_MIN, ceil(T / 64)) frames, one per lane; the last two frames of every block but the last are separators,
// the others its interior.  The band has half-width 2, so interiors do not couple to each other (one level of nested dissection):
//   1. every lane factors its interior A_II = L D L^T (unit lower L, no square roots, no pivoting: a principal submatrix of an SPD
//      matrix) and forward-solves the three right sides z = L^-1 b and its coupling columns V = L^-1 A_IS.  The two columns towards
//      the separators in front fill the whole interior and are stored; the two towards the separators behind are non-zero in the
//      last two rows only and stay in three registers;
//   2. the Schur complement A_SS - V^T D^-1 V on the separators, 2 (P - 1) unknowns of half-width 3, is gathered in LDS in lane
//      order and solved by lane 0 (L D L^T again);
//   3. every lane back-substitutes its interior, X_I = L^-T D^-1 (z - V X_S).
// A track of at most MPL_SMOOTH_SINGLE_MAX frames is one block on lane 0: the same code with no separator.  Order 1 is the same
// code with a zero outer band.  Factors, columns, iterates and the staged inputs live in the workspace as [quantity][row of the
// block][lane], so the lanes of a wave touch consecutive doubles.  fp64 throughout, every output rounded once, sums over a track
// first along each block in frame order and then over the blocks in lane order: no atomics, and the bits of a track depend on its
// own frames only.
#include "common.hpp"
#include "reprojection.hpp"

namespace mpl {
namespace {

constexpr int ST_LANES = MPL_SMOOTH_LANES;
constexpr int ST_Q = MPL_SMOOTH_WS_DOUBLES;
// the quantities of the workspace, each a plane of track_region(T) doubles
enum { Q_DINV = 0, Q_L1 = 1, Q_L2 = 2, Q_V0 = 3, Q_V1 = 4, Q_Z = 5, Q_XA = 8, Q_XB = 11, Q_Y = 14, Q_W = 17 };
static_assert(Q_W + 1 == ST_Q, "MPL_SMOOTH_WS_DOUBLES counts the planes");
// what a lane hands to the Schur system, one LDS row each
enum { S_LL00 = 0, S_LL01, S_LL11, S_LR00, S_LR01, S_LR10, S_LR11, S_RR00, S_RR01, S_RR11, S_GL0 = 10, S_GL1 = 13, S_GR0 = 16, S_GR1 = 19,
       S_A0 = 22, S_A1, S_E, S_B0 = 25, S_B1 = 28, S_ROWS = 31 };
constexpr int ST_UMAX = 2 * (ST_LANES - 1);

struct SmoothParams {
    const float* points;
    const float* weight;
    const int* seg;
    double* ws;
    float *out_points, *out_residual, *out_irls;
    double *out_cost0, *out_cost;
    int* out_iterations;
    unsigned char* out_status;
    double* out_points64;
    double lambda, huber, tol;
    long long T;
    int J, order, max_it, single;
};

// doubles of one plane of one track, and where the planes of segment s start (in planes of one double per frame and joint)
__host__ __device__ inline size_t track_region(size_t T) { return T + T / 64 + 64; }

// the bands of D^T D at frame t of a segment of T frames: diagonal, (t, t+1) and (t, t+2).  Row r of D^2 is (1, -2, 1) on r-1, r,
// r+1 for 1 <= r <= T-2; row r of D^1 is (-1, 1) on r, r+1 for 0 <= r <= T-2
struct Bands { double c0, c1, c2; };
__device__ __forceinline__ Bands bands(int t, int T, int order) {
    Bands b;
    if (order == 2) {
        const double r0 = (t >= 1 && t <= T - 2) ? 1.0 : 0.0, rm = (t >= 2 && t <= T - 1) ? 1.0 : 0.0, rp = (t >= 0 && t <= T - 3) ? 1.0 : 0.0;
        b.c0 = 4.0 * r0 + rm + rp;
        b.c1 = -2.0 * (r0 + rp);
        b.c2 = rp;
    } else {
        const double r0 = (t >= 0 && t <= T - 2) ? 1.0 : 0.0, rm = (t >= 1 && t <= T - 1) ? 1.0 : 0.0;
        b.c0 = r0 + rm;
        b.c1 = -r0;
        b.c2 = 0.0;
    }
    return b;
}

__global__ void __launch_bounds__(ST_LANES) smooth_tracks_kernel(const SmoothParams p) {
    __shared__ double sh[S_ROWS][ST_LANES];
    __shared__ double sl[ST_UMAX][4];          // the Schur factor: L[u][u-1], L[u][u-2], L[u][u-3], 1 / d[u]
    __shared__ double sx[ST_UMAX][3];          // its right sides, then the separators' values
    const int s = blockIdx.x, j = blockIdx.y, lane = threadIdx.x, J = p.J, order = p.order;
    const int t0 = p.seg[s], T = p.seg[s + 1] - t0;
    if (t0 < 0 || T < 1 || T > MPL_SMOOTH_MAX_SEGMENT || (long long)t0 + T > p.T) return;      // a table that is not the host's list
    int L, P;
    if (p.single || T <= MPL_SMOOTH_SINGLE_MAX) {
        L = T;
        P = 1;
    } else {
        L = (T + ST_LANES - 1) / ST_LANES;
        L = L < MPL_SMOOTH_CHUNK_MIN ? MPL_SMOOTH_CHUNK_MIN : L;
        P = (T + L - 1) / L;
    }
    const size_t R = track_region((size_t)T);
    double* const W = p.ws + (size_t)ST_Q * ((size_t)J * ((size_t)t0 + (size_t)t0 / 64 + 64 * (size_t)s) + (size_t)j * R);
    const double lam = p.lambda, h = p.huber, h2 = h * h;
    const size_t frame = (size_t)J * 3;
    const float* const Yp = p.points + ((size_t)t0 * J + j) * 3;
    const float* const Wp = p.weight ? p.weight + (size_t)t0 * J + j : nullptr;
    const size_t o0 = (size_t)t0 * J + j;       // (frame 0 of the track, joint j) in a (T,J) output

    // ---- stage: Y and w in fp64, zero at gaps, in the block layout; frames that take part, their extent
    int cnt = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    #pragma unroll 1
    for (int t = lane; t < T; t += ST_LANES) {
        const float* y = Yp + (size_t)t * frame;
        const double y0 = y[0], y1 = y[1], y2 = y[2], w = Wp ? (double)Wp[(size_t)t * J] : 1.0;
        const bool part = isfinite(y0) && isfinite(y1) && isfinite(y2) && takes_part(w);
        const size_t k = (size_t)(t % L) * P + t / L;
        W[(Q_Y + 0) * R + k] = part ? y0 : 0.0;
        W[(Q_Y + 1) * R + k] = part ? y1 : 0.0;
        W[(Q_Y + 2) * R + k] = part ? y2 : 0.0;
        W[Q_W * R + k] = part ? w : 0.0;
        if (part) {
            ++cnt;
            lo[0] = fmin(lo[0], y0); hi[0] = fmax(hi[0], y0);
            lo[1] = fmin(lo[1], y1); hi[1] = fmax(hi[1], y1);
            lo[2] = fmin(lo[2], y2); hi[2] = fmax(hi[2], y2);
        }
    }
    sh[0][lane] = (double)cnt;
    for (int a = 0; a < 3; ++a) { sh[1 + a][lane] = lo[a]; sh[4 + a][lane] = hi[a]; }
    __syncthreads();
    double total = 0.0, extent = 0.0;
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    #pragma unroll 1
    for (int b = 0; b < ST_LANES; ++b) {
        total += sh[0][b];
        for (int a = 0; a < 3; ++a) { lo[a] = fmin(lo[a], sh[1 + a][b]); hi[a] = fmax(hi[a], sh[4 + a][b]); }
    }
    for (int a = 0; a < 3; ++a) extent = fmax(extent, hi[a] - lo[a]);      // -inf with no frame at all; such a track passes through
    __syncthreads();

    // ---- passed through: nothing to solve (fewer than `order` frames take part: singular) or nothing asked for
    if (total < (double)order || p.max_it == 0) {
        for (int t = lane; t < T; t += ST_LANES) {
            const unsigned int* y = reinterpret_cast<const unsigned int*>(Yp + (size_t)t * frame);
            unsigned int* o = reinterpret_cast<unsigned int*>(p.out_points + (o0 + (size_t)t * J) * 3);
            o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
            const bool part = W[Q_W * R + (size_t)(t % L) * P + t / L] > 0.0;
            p.out_residual[o0 + (size_t)t * J] = part ? 0.0f : NAN;
            p.out_irls[o0 + (size_t)t * J] = part ? 1.0f : 0.0f;
            if (p.out_points64) {
                const float* f = Yp + (size_t)t * frame;
                double* o64 = p.out_points64 + (o0 + (size_t)t * J) * 3;
                o64[0] = f[0]; o64[1] = f[1]; o64[2] = f[2];
            }
        }
        if (lane == 0) {
            const size_t c = (size_t)s * J + j;
            p.out_cost0[c] = 0.0; p.out_cost[c] = 0.0; p.out_iterations[c] = 0; p.out_status[c] = (unsigned char)LM_PASSED_THROUGH;
        }
        return;
    }

    const int p0 = lane * L;                                               // the first frame of this lane's block
    const int len = lane < P ? (T - p0 < L ? T - p0 : L) : 0;               // its frames
    const int n = lane < P - 1 ? L - 2 : len;                               // its interior (>= 6 where separators follow)

    // the weight of frame (row i of this lane's block) in a solve: w, times min(1, h / |X - Y|) at the iterate in planes xq
    auto weight_at = [&](size_t k, int xq) -> double {
        double w = W[Q_W * R + k];
        if (xq >= 0 && w > 0.0) {
            const double r0 = W[(xq + 0) * R + k] - W[(Q_Y + 0) * R + k], r1 = W[(xq + 1) * R + k] - W[(Q_Y + 1) * R + k],
                         r2 = W[(xq + 2) * R + k] - W[(Q_Y + 2) * R + k];
            const double r = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
            if (r > h) w *= h / r;
        }
        return w;
    };

    // ---- one solve: the weights from the iterate in planes `from` (-1: the given weights), the result into planes `to`
    auto solve = [&](int from, int to) {
        double ra = 0.0, rb = 0.0, rc = 0.0;                               // the two columns behind: rows q-1 | q of the first, q of the second
        {
            double dp = 0.0, dpp = 0.0, l1p = 0.0, l1pp = 0.0, l2p = 0.0, l2pp = 0.0, dip = 0.0, dipp = 0.0;
            double yp[5] = {0, 0, 0, 0, 0}, ypp[5] = {0, 0, 0, 0, 0};
            double ll00 = 0, ll01 = 0, ll11 = 0, gl0[3] = {0, 0, 0}, gl1[3] = {0, 0, 0};
            #pragma unroll 1
            for (int i = 0; i < n; ++i) {
                const int t = p0 + i;
                const size_t k = (size_t)i * P + lane;
                const Bands c = bands(t, T, order);
                const double w = weight_at(k, from);
                const double d = (w + lam * c.c0) - l1p * l1p * dp - l2pp * l2pp * dpp;
                const double di = 1.0 / d;
                const double l1 = i + 1 < n ? (lam * c.c1 - l2p * dp * l1p) * di : 0.0;
                const double l2 = i + 2 < n ? lam * c.c2 * di : 0.0;
                double y[5];
                for (int a = 0; a < 3; ++a) y[a] = w * W[(Q_Y + a) * R + k];
                y[3] = (lane > 0 && i == 0) ? lam * bands(t - 2, T, order).c2 : 0.0;
                y[4] = lane > 0 ? (i == 0 ? lam * bands(t - 1, T, order).c1 : i == 1 ? lam * bands(t - 2, T, order).c2 : 0.0) : 0.0;
                for (int a = 0; a < 5; ++a) y[a] = y[a] - l1p * yp[a] - l2pp * ypp[a];
                ll00 += y[3] * y[3] * di; ll01 += y[3] * y[4] * di; ll11 += y[4] * y[4] * di;
                for (int a = 0; a < 3; ++a) { gl0[a] += y[3] * y[a] * di; gl1[a] += y[4] * y[a] * di; }
                W[Q_DINV * R + k] = di; W[Q_L1 * R + k] = l1; W[Q_L2 * R + k] = l2; W[Q_V0 * R + k] = y[3]; W[Q_V1 * R + k] = y[4];
                for (int a = 0; a < 3; ++a) W[(Q_Z + a) * R + k] = y[a];
                dpp = dp; dp = d; dipp = dip; dip = di; l1pp = l1p; l1p = l1; l2pp = l2p; l2p = l2;
                for (int a = 0; a < 5; ++a) { ypp[a] = yp[a]; yp[a] = y[a]; }
            }
            if (P == 1) {
                // no separator: straight to the back-substitution
            } else {
                sh[S_LL00][lane] = ll00; sh[S_LL01][lane] = ll01; sh[S_LL11][lane] = ll11;
                for (int a = 0; a < 3; ++a) { sh[S_GL0 + a][lane] = gl0[a]; sh[S_GL1 + a][lane] = gl1[a]; }
                if (lane < P - 1) {
                    const int q = p0 + n - 1;                               // the last interior frame; q-1 is one too
                    ra = lam * bands(q - 1, T, order).c2;
                    rb = lam * bands(q, T, order).c1 - l1pp * ra;
                    rc = lam * bands(q, T, order).c2;
                    sh[S_RR00][lane] = ra * ra * dipp + rb * rb * dip;
                    sh[S_RR01][lane] = rb * rc * dip;
                    sh[S_RR11][lane] = rc * rc * dip;
                    sh[S_LR00][lane] = ypp[3] * ra * dipp + yp[3] * rb * dip;
                    sh[S_LR01][lane] = yp[3] * rc * dip;
                    sh[S_LR10][lane] = ypp[4] * ra * dipp + yp[4] * rb * dip;
                    sh[S_LR11][lane] = yp[4] * rc * dip;
                    for (int a = 0; a < 3; ++a) {
                        sh[S_GR0 + a][lane] = ypp[a] * ra * dipp + yp[a] * rb * dip;
                        sh[S_GR1 + a][lane] = yp[a] * rc * dip;
                    }
                    // its own two separators: diagonal, their coupling and right sides
                    const size_t k0 = (size_t)(L - 2) * P + lane, k1 = k0 + P;
                    const Bands c0 = bands(p0 + L - 2, T, order), c1 = bands(p0 + L - 1, T, order);
                    const double w0 = weight_at(k0, from), w1 = weight_at(k1, from);
                    sh[S_A0][lane] = w0 + lam * c0.c0;
                    sh[S_A1][lane] = w1 + lam * c1.c0;
                    sh[S_E][lane] = lam * c0.c1;
                    for (int a = 0; a < 3; ++a) { sh[S_B0 + a][lane] = w0 * W[(Q_Y + a) * R + k0]; sh[S_B1 + a][lane] = w1 * W[(Q_Y + a) * R + k1]; }
                }
            }
        }
        if (P > 1) {
            __syncthreads();
            if (lane == 0) {
                const int U = 2 * (P - 1);
                #pragma unroll 1
                for (int u = 0; u < U; ++u) {
                    const int m = u >> 1;
                    double a0, a1, a2, a3, b[3];
                    if ((u & 1) == 0) {
                        a0 = sh[S_A0][m] - sh[S_RR00][m] - sh[S_LL00][m + 1];
                        a1 = m ? -sh[S_LR10][m] : 0.0;
                        a2 = m ? -sh[S_LR00][m] : 0.0;
                        a3 = 0.0;
                        for (int a = 0; a < 3; ++a) b[a] = sh[S_B0 + a][m] - sh[S_GR0 + a][m] - sh[S_GL0 + a][m + 1];
                    } else {
                        a0 = sh[S_A1][m] - sh[S_RR11][m] - sh[S_LL11][m + 1];
                        a1 = sh[S_E][m] - sh[S_RR01][m] - sh[S_LL01][m + 1];
                        a2 = m ? -sh[S_LR11][m] : 0.0;
                        a3 = m ? -sh[S_LR01][m] : 0.0;
                        for (int a = 0; a < 3; ++a) b[a] = sh[S_B1 + a][m] - sh[S_GR1 + a][m] - sh[S_GL1 + a][m + 1];
                    }
                    // row u of L D L^T at half-width 3: d1..d3 the pivots of rows u-1..u-3
                    const double d1 = u >= 1 ? 1.0 / sl[u - 1][3] : 0.0, d2 = u >= 2 ? 1.0 / sl[u - 2][3] : 0.0, d3 = u >= 3 ? 1.0 / sl[u - 3][3] : 0.0;
                    const double l3 = u >= 3 ? a3 * sl[u - 3][3] : 0.0;
                    const double l2 = u >= 2 ? (a2 - l3 * d3 * (u >= 3 ? sl[u - 2][0] : 0.0)) * sl[u - 2][3] : 0.0;
                    const double l1 = u >= 1 ? (a1 - l3 * d3 * (u >= 3 ? sl[u - 1][1] : 0.0) - l2 * d2 * (u >= 2 ? sl[u - 1][0] : 0.0)) * sl[u - 1][3] : 0.0;
                    const double d = a0 - l1 * l1 * d1 - l2 * l2 * d2 - l3 * l3 * d3;
                    sl[u][0] = l1; sl[u][1] = l2; sl[u][2] = l3; sl[u][3] = 1.0 / d;
                    for (int a = 0; a < 3; ++a)
                        sx[u][a] = b[a] - (u >= 1 ? l1 * sx[u - 1][a] : 0.0) - (u >= 2 ? l2 * sx[u - 2][a] : 0.0) - (u >= 3 ? l3 * sx[u - 3][a] : 0.0);
                }
                #pragma unroll 1
                for (int u = U - 1; u >= 0; --u)
                    for (int a = 0; a < 3; ++a)
                        sx[u][a] = sx[u][a] * sl[u][3] - (u + 1 < U ? sl[u + 1][0] * sx[u + 1][a] : 0.0) - (u + 2 < U ? sl[u + 2][1] * sx[u + 2][a] : 0.0)
                                   - (u + 3 < U ? sl[u + 3][2] * sx[u + 3][a] : 0.0);
            }
            __syncthreads();
        }
        if (lane < P) {
            double xl0[3] = {0, 0, 0}, xl1[3] = {0, 0, 0}, xr0[3] = {0, 0, 0}, xr1[3] = {0, 0, 0};
            if (lane > 0)
                for (int a = 0; a < 3; ++a) { xl0[a] = sx[2 * (lane - 1)][a]; xl1[a] = sx[2 * (lane - 1) + 1][a]; }
            if (lane < P - 1) {
                const size_t k0 = (size_t)(L - 2) * P + lane;
                for (int a = 0; a < 3; ++a) {
                    xr0[a] = sx[2 * lane][a]; xr1[a] = sx[2 * lane + 1][a];
                    W[(to + a) * R + k0] = xr0[a]; W[(to + a) * R + k0 + P] = xr1[a];
                }
            }
            double x1[3] = {0, 0, 0}, x2[3] = {0, 0, 0};
            #pragma unroll 1
            for (int i = n - 1; i >= 0; --i) {
                const size_t k = (size_t)i * P + lane;
                const double di = W[Q_DINV * R + k], l1 = W[Q_L1 * R + k], l2 = W[Q_L2 * R + k], v0 = W[Q_V0 * R + k], v1 = W[Q_V1 * R + k];
                for (int a = 0; a < 3; ++a) {
                    double y = W[(Q_Z + a) * R + k] - v0 * xl0[a] - v1 * xl1[a];
                    if (i == n - 1) y -= rb * xr0[a] + rc * xr1[a];
                    if (i == n - 2) y -= ra * xr0[a];
                    const double x = y * di - l1 * x1[a] - l2 * x2[a];
                    W[(to + a) * R + k] = x;
                    x2[a] = x1[a]; x1[a] = x;
                }
            }
        }
        __syncthreads();                                                    // the iterate is complete for every lane
    };

    // ---- E at the iterate in planes xq; the largest coordinate step from the iterate in planes oq (-1: none)
    auto evaluate = [&](int xq, int oq, double& E, double& step) {
        double ed = 0.0, ep = 0.0, st = 0.0;
        if (lane < P) {
            double prev[3] = {0, 0, 0}, cur[3], next[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                if (lane > 0) prev[a] = W[(xq + a) * R + (size_t)(L - 1) * P + lane - 1];
                cur[a] = W[(xq + a) * R + lane];
            }
            #pragma unroll 1
            for (int i = 0; i < len; ++i) {
                const int t = p0 + i;
                const size_t k = (size_t)i * P + lane;
                for (int a = 0; a < 3; ++a)
                    next[a] = i + 1 < len ? W[(xq + a) * R + k + P] : lane + 1 < P ? W[(xq + a) * R + lane + 1] : 0.0;
                const double w = W[Q_W * R + k];
                if (w > 0.0) {
                    const double r0 = cur[0] - W[(Q_Y + 0) * R + k], r1 = cur[1] - W[(Q_Y + 1) * R + k], r2 = cur[2] - W[(Q_Y + 2) * R + k];
                    const double ss = r0 * r0 + r1 * r1 + r2 * r2;
                    ed += w * ((h > 0.0 && ss > h2) ? 2.0 * h * sqrt(ss) - h2 : ss);
                }
                if (order == 2) {
                    if (t >= 1 && t <= T - 2)
                        for (int a = 0; a < 3; ++a) { const double v = next[a] - 2.0 * cur[a] + prev[a]; ep += v * v; }
                } else if (t <= T - 2) {
                    for (int a = 0; a < 3; ++a) { const double v = next[a] - cur[a]; ep += v * v; }
                }
                if (oq >= 0)
                    for (int a = 0; a < 3; ++a) st = fmax(st, fabs(cur[a] - W[(oq + a) * R + k]));
                for (int a = 0; a < 3; ++a) { prev[a] = cur[a]; cur[a] = next[a]; }
            }
        }
        sh[0][lane] = ed; sh[1][lane] = ep; sh[2][lane] = st;
        __syncthreads();
        double sd = 0.0, sp = 0.0;
        step = 0.0;
        #pragma unroll 1
        for (int b = 0; b < P; ++b) { sd += sh[0][b]; sp += sh[1][b]; step = fmax(step, sh[2][b]); }
        E = sd + lam * sp;
        __syncthreads();
    };

    // ---- the loop of the header: one pass in the plain mode
    int cur = Q_XA, nxt = Q_XB, it = 0, status = LM_CONVERGED;
    double E = 0.0, cost0 = 0.0;
    for (;;) {
        double En, step;
        const int to = it ? nxt : cur;
        solve(it ? cur : -1, to);
        evaluate(to, it ? cur : -1, En, step);
        if (++it == 1) {
            E = cost0 = En;
            if (!(h > 0.0 && extent > 0.0)) break;
        } else {
            if (!(En < E)) break;                                           // a tie is rejected: the earlier iterate stays
            E = En;
            cur = to; nxt = to == Q_XA ? Q_XB : Q_XA;
            if (step <= p.tol * extent) break;
        }
        if (it >= p.max_it) { status = LM_CAPPED; break; }
    }

    // ---- outputs, every frame of the track
    for (int t = lane; t < T; t += ST_LANES) {
        const size_t k = (size_t)(t % L) * P + t / L, o = o0 + (size_t)t * J;
        const double x0 = W[(cur + 0) * R + k], x1 = W[(cur + 1) * R + k], x2 = W[(cur + 2) * R + k], w = W[Q_W * R + k];
        p.out_points[o * 3 + 0] = (float)x0; p.out_points[o * 3 + 1] = (float)x1; p.out_points[o * 3 + 2] = (float)x2;
        if (p.out_points64) { p.out_points64[o * 3 + 0] = x0; p.out_points64[o * 3 + 1] = x1; p.out_points64[o * 3 + 2] = x2; }
        if (w > 0.0) {
            const double r0 = x0 - W[(Q_Y + 0) * R + k], r1 = x1 - W[(Q_Y + 1) * R + k], r2 = x2 - W[(Q_Y + 2) * R + k];
            const double r = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
            p.out_residual[o] = (float)r;
            p.out_irls[o] = (h > 0.0 && r > h) ? (float)(h / r) : 1.0f;
        } else {
            p.out_residual[o] = NAN;
            p.out_irls[o] = 0.0f;
        }
    }
    if (lane == 0) {
        const size_t c = (size_t)s * J + j;
        p.out_cost0[c] = cost0; p.out_cost[c] = E; p.out_iterations[c] = it; p.out_status[c] = (unsigned char)status;
    }
}

}  // namespace

size_t smooth_tracks_workspace_bytes(long long T, int J, int S) {
    if (T < 1 || T > MPL_SMOOTH_MAX_FRAMES || J < 1 || J > MPL_SMOOTH_MAX_JOINTS || S < 1 || S > T) return 0;
    return sizeof(double) * (size_t)ST_Q * (size_t)J * ((size_t)T + (size_t)T / 64 + 64 * (size_t)S);
}

int launch_smooth_tracks(const float* points, const float* weight, const int* segments, const int* seg_offsets_dev, int S, long long T,
                         int J, double smoothness, int order, double huber, int max_iterations, double step_tolerance, unsigned flags,
                         void* ws, size_t ws_bytes, float* out_points, float* out_residual, float* out_irls, double* out_cost0,
                         double* out_cost, int* out_iterations, unsigned char* out_status, double* out_points64, hipStream_t s) {
    if (!points || !segments || !seg_offsets_dev || !out_points || !out_residual || !out_irls || !out_cost0 || !out_cost || !out_iterations ||
        !out_status || S <= 0 || T <= 0 || J <= 0)
        return MPL_E_INVALID;
    if (T > MPL_SMOOTH_MAX_FRAMES || J > MPL_SMOOTH_MAX_JOINTS || S > T) return MPL_E_INVALID;
    long long sum = 0;
    for (int i = 0; i < S; ++i) {
        if (segments[i] < 1 || segments[i] > MPL_SMOOTH_MAX_SEGMENT) return MPL_E_INVALID;
        sum += segments[i];
    }
    if (sum != T) return MPL_E_INVALID;
    if (order != 1 && order != 2) return MPL_E_INVALID;
    if (!(smoothness > 0.0) || !(smoothness <= FINITE_MAX)) return MPL_E_UNSUPPORTED;
    if (max_iterations < 0 || max_iterations > 1000 || !(step_tolerance >= 0.0) || !(step_tolerance <= FINITE_MAX)) return MPL_E_UNSUPPORTED;
    if (flags & ~(unsigned)MPL_SMOOTH_F_SINGLE_LANE) return MPL_E_INVALID;
#ifndef MPL_LAB
    if (flags & MPL_SMOOTH_F_SINGLE_LANE) return MPL_E_UNSUPPORTED;          // a laboratory measurement, not a mode of the product
#endif
    const size_t need = smooth_tracks_workspace_bytes(T, J, S);
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 7)) return MPL_E_WORKSPACE;
    SmoothParams p;
    p.points = points; p.weight = weight; p.seg = seg_offsets_dev; p.ws = static_cast<double*>(ws);
    p.out_points = out_points; p.out_residual = out_residual; p.out_irls = out_irls; p.out_cost0 = out_cost0; p.out_cost = out_cost;
    p.out_iterations = out_iterations; p.out_status = out_status; p.out_points64 = out_points64;
    p.lambda = smoothness;
    p.huber = huber > 0.0 && huber <= FINITE_MAX ? huber : 0.0;             // <= 0, NaN or inf: the plain cost
    p.tol = step_tolerance;
    p.T = T; p.J = J; p.order = order; p.max_it = max_iterations; p.single = (flags & MPL_SMOOTH_F_SINGLE_LANE) ? 1 : 0;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(smooth_tracks_kernel, dim3((unsigned)S, (unsigned)J), dim3(ST_LANES), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
