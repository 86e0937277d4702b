// Refinement of whole poses by reprojection error under bone-length constraints (mpl_refine_poses).
//
// refine.hip moves every joint on its own; here the J joints of a pose are one body on a tree with bones of known length:
// E(X) = sum_{v,j} w_vj rho(|proj_v(X_j) - px_vj|^2) + bone_weight sum_{live bones j} ((|X_j - X_p(j)| - L_j) / L_j)^2, minimised by
// Levenberg-Marquardt over the 3 J' unknowns of the joints that take part.  The first sum is the cost of refine.hip to the letter
// (views.hpp, takes_part, the Huber weights); the bone term is always quadratic.  The reference has no such step.
//
// One wave per pose, workgroups of one wave, lane j owns joint j: its point, its 3x3 diagonal block, the block of its bone to its
// parent (-c u u^T, kept as the unit vector u and the scalar c) and its slice of g.  The views run in a wave-uniform loop per lane as
// in refine.hip.  The normal matrix has one block per joint and one per bone on a tree, so children are eliminated before their
// parents, level by level, without fill-in: a child hands its parent two scalars beside u, and the solve is O(J) 3x3 operations.  A
// parent reads its children through cross-lane moves, walking them in index order (first child, next sibling), so every sum has one
// order.  E, the smallest depth and the largest step are reduced by butterflies whose result is the same bits in every lane, so
// lambda, the trial count and the status of the pose are wave-uniform.  fp64 on the fp32 tensors, every output rounded once, no LDS,
// no atomics: identical bits from run to run and from batching to batching.  The loop makes at most max_iterations passes.
#include "common.hpp"
#include "reprojection.hpp"

namespace mpl {

namespace {

constexpr int POSE_LANES = 64;          // one wave; joints <= 64

// the tree as the lanes read it: every table is indexed by the joint; lanes at or beyond `joints` have no parent and no child
struct PoseTree {
    signed char parent[POSE_LANES], first_child[POSE_LANES], next_sibling[POSE_LANES];     // -1: none
    unsigned char depth[POSE_LANES];
    int n_levels, max_children;
};

struct PoseParams {
    const float* points;      // (B,J,3)
    const float* px;          // (B,V,J,2)
    const float* conf;        // (B,V,J) or null
    const double* cams;       // device (V,16)
    const double* dist;       // device (V,5) or null
    const float* limb;        // (J,) with limb_stride 0, or (B,J) with limb_stride >= J
    float* out_points;        // (B,J,3)
    float* out_error;         // (B,J)
    float* out_bone;          // (B,J) or null
    double* out_cost0;        // (B,) or null
    double* out_cost;         // (B,) or null
    int* out_iterations;      // (B,) or null
    unsigned char* out_status;    // (B,) or null
    double huber, tol, bone_weight;
    long long limb_stride;
    int V, J, max_it;
    PoseTree tree;
};

// the lane's view of its observations: view v of joint j of pose b sits at element (b V + v) J + j
struct PoseItem {
    const PoseParams& p;
    unsigned base;            // b V J + j; batch * views * joints <= 2^30, so an observation's index (and twice it) fits 32 bits
    __device__ unsigned at(int v) const { return base + (unsigned)(v * p.J); }
    __device__ double weight(int v) const { return p.conf ? (double)p.conf[at(v)] : 1.0; }
};

// what one evaluation leaves in a lane: the pose's cost E and smallest depth (the same bits in every lane once reduced), the lane's
// diagonal block H (xx xy xz yy yz zz) and slice of g, and its bone: the unit vector u child - parent, c = bone_weight / L^2 and
// gr = bone_weight r / L, all zero for a bone that is not live
struct PoseEval {
    double E = 0, H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, u[3] = {0, 0, 0}, c = 0, gr = 0, zmin = __builtin_inf();
    bool behind = false;
};

// r = proj_v(X) - px_v in pixels and the lens jet at the point, as refine.hip states it; false: z_cam <= CAMERA_Z_MIN (or not a number)
template <bool LENS>
__device__ __forceinline__ bool pose_residual(const PoseItem& it, int v, const double X[3], double& r0, double& r1, double& y0, double& y1,
                                              double& zc, LensJet& jet) {
    const double* c = it.p.cams + (size_t)v * 16;
    const Camera cam{c};
    double xc, yc;
    camera_coords(c, X[0], X[1], X[2], xc, yc, zc);
    y0 = xc / zc;
    y1 = yc / zc;
    // the lens row goes through vector registers (a per-lane zero the compiler cannot see through), as in refine.hip, to spare the
    // scalar file
    jet = distort_jet(y0, y1, distortion_of(LENS ? it.p.dist : nullptr, v + (int)(it.base >> 30)));
    const float* q = it.p.px + it.at(v) * 2u;
    r0 = (cam.fx() * jet.x + cam.cx()) - (double)q[0];
    r1 = (cam.fy() * jet.y + cam.cy()) - (double)q[1];
    return zc > CAMERA_Z_MIN;
}

// the lane's own part of an evaluation: its views, and its bone to the parent's point Xp (live: the bone counts)
template <bool LENS>
__device__ __forceinline__ PoseEval pose_eval(const PoseItem& it, unsigned mask, const double X[3], const double Xp[3], bool live, double L,
                                              double inv_L) {
    PoseEval e;
    const double huber = it.p.huber;
    for (int v = 0; v < it.p.V; ++v) {
        if (!(mask >> v & 1u)) continue;
        double r0, r1, y0, y1, zc;
        LensJet jet;
        e.behind |= !pose_residual<LENS>(it, v, X, r0, r1, y0, y1, zc, jet);
        e.zmin = fmin(e.zmin, zc);
        const Camera cam{it.p.cams + (size_t)v * 16};
        const double w = it.weight(v), s = r0 * r0 + r1 * r1;
        const double rn = sqrt(s);
        const bool tail = huber > 0.0 && s > huber * huber;
        e.E += w * (tail ? 2.0 * huber * rn - huber * huber : s);
        const double wi = tail ? w * (huber / rn) : w;
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
    if (live) {
        // r = (|d| - L) / L; d r / d X_j = u / L, d r / d X_p = -u / L; |d| = 0: the residual counts, its gradient is zero
        const double d[3] = {X[0] - Xp[0], X[1] - Xp[1], X[2] - Xp[2]};
        const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), r = (n - L) * inv_L, bw = it.p.bone_weight;
        const double inv_n = n > 0.0 ? 1.0 / n : 0.0;
        e.E += bw * r * r;
#pragma unroll
        for (int k = 0; k < 3; ++k) e.u[k] = d[k] * inv_n;
        e.c = bw * inv_L * inv_L;
        e.gr = bw * r * inv_L;
    }
    return e;
}

// H += s u u^T on the six entries of a symmetric block
__device__ __forceinline__ void add_outer(double H[6], double s, const double u[3]) {
    H[0] += s * (u[0] * u[0]);
    H[1] += s * (u[0] * u[1]);
    H[2] += s * (u[0] * u[2]);
    H[3] += s * (u[1] * u[1]);
    H[4] += s * (u[1] * u[2]);
    H[5] += s * (u[2] * u[2]);
}

// One step of a lane's walk over its children, in index order: the five values `v` of the child `ch`, and the walk moves on to the
// child's next sibling.  false: no child left.  Every lane of the wave makes the same cross-lane moves; a lane without a child
// reads itself.
__device__ __forceinline__ bool child_read(int& ch, int lane, int next_sibling, const double (&v)[5], double (&out)[5]) {
    const bool has = ch >= 0;
    const int src = has ? ch : lane;
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = __shfl(v[k], src);
    const int nx = __shfl(next_sibling, src);
    ch = has ? nx : -1;
    return has;
}

// butterflies: the same bits in every lane, in one order whatever the batch
__device__ __forceinline__ double wave_sum(double v) {
    for (int m = POSE_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int m = POSE_LANES / 2; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
    return v;
}
// the larger of two, a NaN winning: a step that is not a number is no small step
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double wave_nan_max(double v) {
    for (int m = POSE_LANES / 2; m >= 1; m >>= 1) v = nan_max(v, __shfl_xor(v, m));
    return v;
}

// A = L D L^T of a symmetric 3x3 block without pivoting, and A x = b from it; a pivot that is not positive and finite gives NaN.
// Three reciprocals per block, whatever the number of right-hand sides: an fp64 division is a chain of a dozen dependent
// instructions, and at one wave per SIMD nothing hides it.
struct Ldl3 {
    double i0, i1, i2, l10, l20, l21;                       // 1 / d
    bool ok;
    __device__ __forceinline__ explicit Ldl3(const double A[6]) {
        const double d0 = A[0];
        i0 = 1.0 / d0;
        l10 = A[1] * i0;
        l20 = A[2] * i0;
        const double d1 = A[3] - l10 * A[1], t = A[4] - l20 * A[1];
        i1 = 1.0 / d1;
        l21 = t * i1;
        const double d2 = A[5] - l20 * A[2] - l21 * t;
        i2 = 1.0 / d2;
        ok = d0 > 0.0 && d1 > 0.0 && d2 > 0.0 && d0 <= FINITE_MAX && d1 <= FINITE_MAX && d2 <= FINITE_MAX;
    }
    __device__ __forceinline__ void solve(const double b[3], double x[3]) const {
        const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = b[2] - l20 * y0 - l21 * y1;
        const double x2 = y2 * i2, x1 = y1 * i1 - l21 * x2, x0 = y0 * i0 - l10 * x1 - l20 * x2;
        const double nan = __builtin_nan("");
        x[0] = ok ? x0 : nan;
        x[1] = ok ? x1 : nan;
        x[2] = ok ? x2 : nan;
    }
};

// what a lane knows of the tree
struct PoseLane {
    int lane, parent, psrc, first_child, next_sibling, depth;     // psrc: the parent's lane, the lane itself at a root
};

// (H + lambda diag H) delta = -g on the tree.  Deepest level first, a joint j with the block -c u u^T to its parent solves
// y = D_j^-1 rhs_j and z = D_j^-1 u and leaves its parent D_p -= c^2 (u.z) u u^T, rhs_p += c (u.y) u; then root first,
// delta_j = y + c (u.delta_p) z.  A joint that takes no part has delta = 0 and hands nothing on.
__device__ __forceinline__ void pose_step(const PoseTree& tree, const PoseLane& t, bool part, const PoseEval& e, double lambda, double delta[3]) {
    double D[6] = {e.H[0] + lambda * e.H[0], e.H[1], e.H[2], e.H[3] + lambda * e.H[3], e.H[4], e.H[5] + lambda * e.H[5]};
    double rhs[3] = {-e.g[0], -e.g[1], -e.g[2]}, y[3] = {0, 0, 0}, z[3] = {0, 0, 0};
    const bool tied = part && e.c > 0.0;
    double up[5] = {e.u[0], e.u[1], e.u[2], 0.0, 0.0};       // u, a = c^2 (u.z), b = c (u.y)
    for (int lev = tree.n_levels - 1; lev >= 0; --lev) {
        if (t.depth == lev && part) {
            const Ldl3 f(D);
            f.solve(rhs, y);
            if (tied) {
                f.solve(e.u, z);
                up[3] = e.c * e.c * (e.u[0] * z[0] + e.u[1] * z[1] + e.u[2] * z[2]);
                up[4] = e.c * (e.u[0] * y[0] + e.u[1] * y[1] + e.u[2] * y[2]);
            }
        }
        if (lev == 0) break;
        int ch = t.first_child;
        for (int k = 0; k < tree.max_children; ++k) {
            double o[5];
            if (child_read(ch, t.lane, t.next_sibling, up, o) && t.depth == lev - 1) {
                add_outer(D, -o[3], o);
#pragma unroll
                for (int q = 0; q < 3; ++q) rhs[q] += o[4] * o[q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) delta[q] = y[q];
    for (int lev = 1; lev < tree.n_levels; ++lev) {
        const double dp[3] = {__shfl(delta[0], t.psrc), __shfl(delta[1], t.psrc), __shfl(delta[2], t.psrc)};
        if (t.depth == lev && tied) {
            const double s = e.c * (e.u[0] * dp[0] + e.u[1] * dp[1] + e.u[2] * dp[2]);
#pragma unroll
            for (int q = 0; q < 3; ++q) delta[q] = y[q] + s * z[q];
        }
    }
}

}  // namespace

template <bool LENS>
__global__ __launch_bounds__(POSE_LANES) void refine_poses_kernel(const PoseParams p) {
    const int b = blockIdx.x, lane = threadIdx.x, V = p.V, J = p.J;
    const bool in = lane < J;                                // lanes beyond the pose load and store nothing and take no part
    const int j = in ? lane : 0;
    PoseLane t;
    t.lane = lane;
    t.parent = p.tree.parent[lane];
    t.psrc = t.parent >= 0 ? t.parent : lane;
    t.first_child = p.tree.first_child[lane];
    t.next_sibling = p.tree.next_sibling[lane];
    t.depth = p.tree.depth[lane];
    const PoseItem it{p, (unsigned)(b * V * J + j)};
    const float nan = __builtin_nanf("");
    const size_t at = (size_t)b * J + j;
    float x0 = nan, x1 = nan, x2 = nan, Lf = nan;
    unsigned mask = 0;
    int n = 0;
    if (in) {
        x0 = p.points[at * 3];
        x1 = p.points[at * 3 + 1];
        x2 = p.points[at * 3 + 2];
        if (t.parent >= 0) Lf = p.limb[(size_t)b * p.limb_stride + j];
        // the views that take part: a finite weight > 0 and two finite pixel coordinates
        for (int v = 0; v < V; ++v) {
            const double w = it.weight(v);
            const float* q = p.px + it.at(v) * 2u;
            const bool on = takes_part(w) && isfinite(q[0]) && isfinite(q[1]);
            mask |= (unsigned)on << v;
            n += on;
        }
    }
    // A bone is live when both ends have a finite point and a participating view and L is finite and > 0; a joint takes part with
    // two views, or with one and a live bone (its own or a child's).  Both ends of a live bone take part.
    const double L = (double)Lf;
    const bool anchored = isfinite(x0) && isfinite(x1) && isfinite(x2) && n > 0;
    const bool live = t.parent >= 0 && anchored && __shfl((int)anchored, t.psrc) != 0 && L > 0.0 && L <= FINITE_MAX;
    const double inv_L = live ? 1.0 / L : 0.0;
    bool tied = live;
    {
        int ch = t.first_child;
        for (int k = 0; k < p.tree.max_children; ++k) {
            const bool has = ch >= 0;
            const int src = has ? ch : lane;
            const int cl = __shfl((int)live, src), nx = __shfl(t.next_sibling, src);
            tied |= has && cl != 0;
            ch = has ? nx : -1;
        }
    }
    const bool part = anchored && (n >= 2 || tied);
    if (!part) mask = 0;
    const bool any_part = __ballot(part) != 0ull;

    // One call site of the evaluation: the first pass of the loop evaluates the given pose, every later one a trial step.  What
    // decides (E, the depths, the step) is the same bits in every lane, so the loop is wave-uniform.
    double X[3] = {part ? (double)x0 : 0.0, part ? (double)x1 : 0.0, part ? (double)x2 : 0.0};
    double Xt[3] = {X[0], X[1], X[2]}, delta[3] = {0, 0, 0}, lambda = LM_LAMBDA0, E0 = 0;
    PoseEval cur;
    bool valid = true, first = true;
    int status = LM_INVALID, trials = 0;
    while (true) {
        const double Xp[3] = {__shfl(Xt[0], t.psrc), __shfl(Xt[1], t.psrc), __shfl(Xt[2], t.psrc)};
        PoseEval tr = pose_eval<LENS>(it, mask, Xt, Xp, live, L, inv_L);
        {   // the lane's own bone, then the parent's share of its children's bones, in index order
            const double own[5] = {tr.u[0], tr.u[1], tr.u[2], tr.c, tr.gr};
            add_outer(tr.H, tr.c, tr.u);
#pragma unroll
            for (int q = 0; q < 3; ++q) tr.g[q] += tr.gr * tr.u[q];
            int ch = t.first_child;
            for (int k = 0; k < p.tree.max_children; ++k) {
                double o[5];
                if (child_read(ch, lane, t.next_sibling, own, o)) {
                    add_outer(tr.H, o[3], o);
#pragma unroll
                    for (int q = 0; q < 3; ++q) tr.g[q] -= o[4] * o[q];
                }
            }
        }
        tr.E = wave_sum(tr.E);
        tr.zmin = wave_min(tr.zmin);
        const bool behind = __any((int)tr.behind) != 0;
        if (first) {
            first = false;
            valid = !behind;
            if (!valid) break;
            cur = tr;
            E0 = tr.E;
            status = LM_PASSED_THROUGH;
            if (!any_part || p.max_it == 0) break;
            status = LM_CAPPED;
        } else {
            ++trials;
            // strictly lower, and every participating joint in front of its cameras; a cost that is not a number is never accepted
            const bool accept = __builtin_amdgcn_readfirstlane((int)(!behind && tr.E < cur.E)) != 0;
            if (accept) {
                cur = tr;
#pragma unroll
                for (int k = 0; k < 3; ++k) X[k] = Xt[k];
                lambda = fmax(lambda / 10.0, LM_LAMBDA_MIN);
            } else {
                lambda *= 10.0;
            }
            const double step = wave_nan_max(nan_max(fabs(delta[0]), nan_max(fabs(delta[1]), fabs(delta[2]))));
            if (__builtin_amdgcn_readfirstlane((int)(step <= p.tol * cur.zmin)) != 0) {
                status = LM_CONVERGED;
                break;
            }
            if (lambda > LM_LAMBDA_MAX || trials >= p.max_it) break;
        }
        pose_step(p.tree, t, part, cur, lambda, delta);
#pragma unroll
        for (int k = 0; k < 3; ++k) Xt[k] = X[k] + delta[k];
    }

    // the scores at the final pose: the plain weighted root mean square of |r_v| per joint, |d| - L per live bone
    const double Xp[3] = {__shfl(X[0], t.psrc), __shfl(X[1], t.psrc), __shfl(X[2], t.psrc)};
    double S = 0, W = 0;
    if (valid)
        for (int v = 0; v < V; ++v) {
            if (!(mask >> v & 1u)) continue;
            double r0, r1, y0, y1, zc;
            LensJet jet;
            pose_residual<LENS>(it, v, X, r0, r1, y0, y1, zc, jet);
            const double w = it.weight(v);
            S += w * (r0 * r0 + r1 * r1);
            W += w;
        }
    if (in) {
        // a joint that takes no part, or a pose of which no trial was accepted: the given bits
        float* po = p.out_points + at * 3;
        po[0] = !valid ? nan : part ? (float)X[0] : x0;
        po[1] = !valid ? nan : part ? (float)X[1] : x1;
        po[2] = !valid ? nan : part ? (float)X[2] : x2;
        p.out_error[at] = valid && part ? (float)sqrt(S / W) : nan;
        if (p.out_bone) {
            const double d[3] = {X[0] - Xp[0], X[1] - Xp[1], X[2] - Xp[2]};
            p.out_bone[at] = valid && live ? (float)(sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - L) : nan;
        }
    }
    if (lane == 0) {
        const double dnan = __builtin_nan("");
        if (p.out_cost0) p.out_cost0[b] = valid ? E0 : dnan;
        if (p.out_cost) p.out_cost[b] = valid ? cur.E : dnan;
        if (p.out_iterations) p.out_iterations[b] = trials;
        if (p.out_status) p.out_status[b] = (unsigned char)status;
    }
}

namespace {

// parents -> the tables of the lanes; false unless it is one tree: exactly one root, every other parent a joint, no cycle
bool pose_tree_build(const int* parents, int J, PoseTree& t) {
    int roots = 0;
    for (int j = 0; j < J; ++j) {
        if (parents[j] == -1) ++roots;
        else if (parents[j] < 0 || parents[j] >= J || parents[j] == j) return false;
    }
    if (roots != 1) return false;
    int deepest = 0;
    for (int j = 0; j < POSE_LANES; ++j) {
        t.parent[j] = t.first_child[j] = t.next_sibling[j] = -1;
        t.depth[j] = 0;
    }
    for (int j = 0; j < J; ++j) {
        int d = 0;
        for (int k = j; parents[k] != -1; k = parents[k])
            if (++d >= J) return false;
        t.parent[j] = (signed char)parents[j];
        t.depth[j] = (unsigned char)d;
        deepest = d > deepest ? d : deepest;
    }
    t.max_children = 0;
    for (int q = 0; q < J; ++q) {
        int last = -1, count = 0;
        for (int c = 0; c < J; ++c) {
            if (parents[c] != q) continue;
            if (last < 0) t.first_child[q] = (signed char)c;
            else t.next_sibling[last] = (signed char)c;
            last = c;
            ++count;
        }
        t.max_children = count > t.max_children ? count : t.max_children;
    }
    t.n_levels = deepest + 1;
    return true;
}

}  // namespace

int launch_refine_poses(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                        const float* limb, long long limb_stride, const int* parents, int B, int V, int J, double huber,
                        double bone_weight, int max_iterations, double step_tolerance, float* out_points, float* out_error,
                        float* out_bone_error, double* out_cost0, double* out_cost, int* out_iterations, unsigned char* out_status,
                        hipStream_t s) {
    if (!limb || !parents) return MPL_E_INVALID;
    if (const int e = refine_args_check(points, pixels, cams_dev, out_points, out_error, B, V, J, max_iterations, step_tolerance)) return e;
    if (limb_stride != 0 && limb_stride < J) return MPL_E_INVALID;
    if (!(bone_weight >= 0.0) || !(bone_weight <= FINITE_MAX)) return MPL_E_UNSUPPORTED;
    PoseParams p;
    if (!pose_tree_build(parents, J, p.tree)) return MPL_E_INVALID;
    p.points = points; p.px = pixels; p.conf = conf; p.cams = cams_dev; p.dist = dist_dev; p.limb = limb;
    p.out_points = out_points; p.out_error = out_error; p.out_bone = out_bone_error; p.out_cost0 = out_cost0; p.out_cost = out_cost;
    p.out_iterations = out_iterations; p.out_status = out_status;
    p.huber = huber > 0.0 ? huber : 0.0;                 // <= 0 or NaN: the plain cost
    p.tol = step_tolerance;
    p.bone_weight = bone_weight;
    p.limb_stride = limb_stride;
    p.V = V; p.J = J; p.max_it = max_iterations;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dist_dev)
        hipLaunchKernelGGL(refine_poses_kernel<true>, dim3((unsigned)B), dim3(POSE_LANES), 0, s, p);
    else
        hipLaunchKernelGGL(refine_poses_kernel<false>, dim3((unsigned)B), dim3(POSE_LANES), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
