// Recursive pictorial structure model on the device: a 3D pose from whole detector heatmaps, by max-product over a tree of joints
// under limb-length constraints on a grid around the root, refined by rounds of small grids around every joint.
//
// Reference (MPL/lib/multiviews/pictorial.py, the numpy file): compute_grid :106-117, compute_unary_term :144-188,
// compute_pairwise_constrain :120-141, infer :18-84, recursive_infer :191-209, rpsm :212-247; the projection is
// cameras.py:22-46 and the crop is utils/transforms.py:61-94 with rot = 0, written in closed form.  The semantics, the two
// deviations and the envelope are written down in include/mpl_hip.h (mpl_rpsm).  fp64 throughout, no atomics on floating-point
// values, every reduction merged by one total order (NaN, then value, then lower index): identical bits run to run and batch to batch.
//
// Launches: 2 + the number of tree levels that have children (7 for the 17-joint body), whatever the batch and recur_depth.
//   rpsm_unary_kernel   one thread per (pose, group of 8 joints, bin of the first grid): the bin is projected once per view and
//                       the view's maps of the group are sampled bilinearly; a joint's energies start as its unary term.
//   rpsm_level_kernel   one launch per tree level, deepest parents first; a workgroup owns 256 bins of one parent joint of one pose
//                       and, child after child, keeps the child's energies (n^3 doubles, 32 KiB at 16^3) in LDS while every
//                       thread scans them for its own parent bin.  On the shared regular grid a pair is allowed by
//                       m = dix^2 + diy^2 + diz^2 alone, and the allowed m form one interval [lo, hi], found per edge by
//                       evaluating | sqrt(m) step - limb | <= tolerance for every m: the pair test is one multiply-add, one
//                       subtraction and one unsigned compare, and a row of n child bins that no lane of the wave can reach
//                       (dix^2 + diy^2 > hi) is skipped by one ballot.  Disallowed pairs contribute the candidate 0.0: its first
//                       index is found by a scan that stops at the first disallowed pair and merged in afterwards.  A child
//                       with a NaN among its energies (rare) takes the plain scan that applies the total order pair by pair.
//                       The parent's energy times the maximum goes back in place, the argmax into the back-pointer table.
//   rpsm_final_kernel   one workgroup per pose: root argmax, the walk down the back-pointers, then all recur_depth rounds
//                       (unary on each joint's own grid, pairwise by the norm between the two grids, the same inference) with the
//                       state in LDS and no trip to the host.
#include "common.hpp"
#include "views.hpp"

namespace mpl {

constexpr int RPSM_MAX_J = 64;
constexpr int RPSM_MAX_BINS = 4096;          // 16^3: a joint's energies fill 32 KiB of LDS
constexpr int RPSM_MAX_RBINS = 64;           // 4^3
constexpr int RPSM_EMPTY = 0x7fffffff;
constexpr int RPSM_JG = 8;                   // joints per thread of the unary kernel

struct RpsmTree {                            // built on the host from `parents`
    signed char parent[RPSM_MAX_J];
    unsigned char order[RPSM_MAX_J];         // the joints by depth, the root first
    unsigned char level_start[RPSM_MAX_J + 1];   // order[level_start[d] .. level_start[d + 1]): the joints of depth d
    unsigned char child_start[RPSM_MAX_J + 1];   // child[child_start[j] .. child_start[j + 1]): the children of j, ascending
    unsigned char child[RPSM_MAX_J];
    int n_levels;
};

struct RpsmParams : HeatmapTable {
    const float* center;
    const float* scale;
    const double* cams;
    const double* dist;                      // (V,5) k1 k2 k3 p1 p2, or null
    const float* root_center;
    const float* limb;
    long long limb_stride;                   // 0: one (J,) row for every pose
    double* ws_energy;                       // (B,J,nb)
    unsigned short* ws_back;                 // (B,J,nb): the child's bin per parent bin, at the child's row
    float* poses;
    int* bins;
    double* energy;
    int n, nb, rn, rnb, depth;
    double img_w, img_h, grid_size, tol;
    RpsmTree tree;
};

// np.linspace(-size / 2, size / 2, n)[i] + centre, with numpy's roundings: i * step + start in two steps, the last point the stop
__device__ __forceinline__ double rpsm_coord(int i, int n, double size, double centre) {
#pragma clang fp contract(off)
    const double stop = size * 0.5, step = size / (double)(n - 1);
    const double scaled = (double)i * step;
    const double l = i == n - 1 ? stop : scaled + -stop;
    return l + centre;
}

// bin (iy * n + ix) * n + iz of the grid of n^3 points of extent `size` about c: meshgrid's default xy indexing
__device__ __forceinline__ void rpsm_point(int bin, int n, double size, const double* c, double& X, double& Y, double& Z) {
    const int iz = bin % n, ix = (bin / n) % n, iy = bin / (n * n);
    X = rpsm_coord(ix, n, size, c[0]);
    Y = rpsm_coord(iy, n, size, c[1]);
    Z = rpsm_coord(iz, n, size, c[2]);
}

// the heatmap cell coordinates of a world point in view v of pose b; false where the point is not in front of the camera
__device__ __forceinline__ bool rpsm_project(const RpsmParams& p, int b, int v, double X, double Y, double Z, double& ux, double& uy) {
    const Camera cam{p.cams + (size_t)v * 16};
    double xc, yc, zc;
    camera_coords(cam.c, X, Y, Z, xc, yc, zc);
    if (zc <= CAMERA_Z_MIN) return false;
    const Normalized yd = distort_normalized(xc / zc, yc / zc, distortion_of(p.dist, v));   // a null table: the pinhole, bit for bit
    const Pixel px = pixel_of(cam, yd.x, yd.y);
    const size_t bv = ((size_t)b * p.V + v) * 2;
    const double k = p.img_w / (200.0 * (double)p.scale[bv]);
    ux = ((px.x - (double)p.center[bv]) * k + p.img_w * 0.5) * (double)p.W / p.img_w;
    uy = ((px.y - (double)p.center[bv + 1]) * k + p.img_h * 0.5) * (double)p.H / p.img_h;
    return true;
}

// bilinear value of an (H,W) map at (ux, uy) in cells, 0 outside [0, W-1] x [0, H-1] (the borders are inside)
__device__ __forceinline__ double rpsm_sample(const void* map, int dt, int H, int W, double ux, double uy) {
    if (!(ux >= 0.0 && ux <= (double)(W - 1) && uy >= 0.0 && uy <= (double)(H - 1))) return 0.0;
    int x0 = (int)ux, y0 = (int)uy;
    if (x0 > W - 2) x0 = W - 2;
    if (y0 > H - 2) y0 = H - 2;
    const double tx = ux - (double)x0, ty = uy - (double)y0, sx = 1.0 - tx, sy = 1.0 - ty;
    const size_t o = (size_t)y0 * (size_t)W + (size_t)x0;
    const double v00 = hm_fetch(map, o, dt), v10 = hm_fetch(map, o + 1, dt);                  // v<x><y>
    const double v01 = hm_fetch(map, o + W, dt), v11 = hm_fetch(map, o + W + 1, dt);
    return ((v00 * (sx * sy) + v01 * (sx * ty)) + v10 * (tx * sy)) + v11 * (tx * ty);
}

// a is ahead of b: a candidate at all, then NaN above everything, then the value, then the lower index
__device__ __forceinline__ bool rpsm_ahead(double av, int ai, double bv, int bi) {
    if (ai == RPSM_EMPTY) return false;
    if (bi == RPSM_EMPTY) return true;
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

__global__ __launch_bounds__(256) void rpsm_unary_kernel(const RpsmParams p) {
    const int nblk = (p.nb + 255) / 256, groups = (p.J + RPSM_JG - 1) / RPSM_JG;
    const int blk = (int)(blockIdx.x % (unsigned)nblk), rest = (int)(blockIdx.x / (unsigned)nblk);
    const int jg = rest % groups, b = rest / groups;
    const int bin = blk * 256 + (int)threadIdx.x;
    if (bin >= p.nb || b >= p.B) return;
    const double c[3] = {(double)p.root_center[(size_t)b * 3], (double)p.root_center[(size_t)b * 3 + 1], (double)p.root_center[(size_t)b * 3 + 2]};
    double X, Y, Z;
    rpsm_point(bin, p.n, p.grid_size, c, X, Y, Z);
    double acc[RPSM_JG];
#pragma unroll
    for (int k = 0; k < RPSM_JG; ++k) acc[k] = 0.0;
    for (int v = 0; v < p.V; ++v) {
        double ux, uy;
        if (!rpsm_project(p, b, v, X, Y, Z, ux, uy)) continue;
#pragma unroll
        for (int k = 0; k < RPSM_JG; ++k) {
            const int j = jg * RPSM_JG + k;
            if (j < p.J) acc[k] += rpsm_sample(p.map(b, v, j), p.dtype, p.H, p.W, ux, uy);
        }
    }
#pragma unroll
    for (int k = 0; k < RPSM_JG; ++k) {
        const int j = jg * RPSM_JG + k;
        if (j < p.J) p.ws_energy[((size_t)b * p.J + j) * (size_t)p.nb + bin] = acc[k];
    }
}

// U child bins of one row, all of them loaded before the first compare: bin jbase + k has dz = dz0 - k, and m - lo = mxy_lo + dz^2
template <int U>
__device__ __forceinline__ void rpsm_chunk(const double* row, int jbase, int dz0, int mxy_lo, unsigned span, double& best, int& idx) {
    double e[U];
#pragma unroll
    for (int k = 0; k < U; ++k) e[k] = row[k];
#pragma unroll
    for (int k = 0; k < U; ++k) {
        const int dz = dz0 - k;
        if ((unsigned)(__mul24(dz, dz) + mxy_lo) <= span && e[k] > best) { best = e[k]; idx = jbase + k; }
    }
}

__global__ __launch_bounds__(256) void rpsm_level_kernel(const RpsmParams p, int level) {
    __shared__ double se[RPSM_MAX_BINS];
    __shared__ int s_lo, s_hi, s_nan;
    const int tid = (int)threadIdx.x, n = p.n, nb = p.nb;
    const int nblk = (nb + 255) / 256, first = p.tree.level_start[level], cnt = p.tree.level_start[level + 1] - first;
    const int blk = (int)(blockIdx.x % (unsigned)nblk), rest = (int)(blockIdx.x / (unsigned)nblk);
    const int node = p.tree.order[first + rest % cnt], b = rest / cnt;
    const int c_begin = p.tree.child_start[node], c_end = p.tree.child_start[node + 1];
    if (c_begin == c_end || b >= p.B) return;                                    // a leaf keeps its unary term: nothing to do
    const int i = blk * 256 + tid;
    const bool live = i < nb;
    const int ii = live ? i : 0;
    const int iz = ii % n, ix = (ii / n) % n, iy = ii / (n * n);
    double* eb = p.ws_energy + (size_t)b * p.J * (size_t)nb;
    double acc = eb[(size_t)node * nb + ii];
    const double step = p.grid_size / (double)(n - 1);
    const int m_max = 3 * (n - 1) * (n - 1);
    for (int ci = c_begin; ci < c_end; ++ci) {
        const int c = p.tree.child[ci];
        __syncthreads();                                                         // the scan of the child before is over
        if (tid == 0) { s_lo = RPSM_EMPTY; s_hi = -1; s_nan = 0; }
        bool nan = false;
        for (int j = tid; j < nb; j += 256) {
            const double e = eb[(size_t)c * nb + j];
            se[j] = e;
            nan |= e != e;
        }
        __syncthreads();
        if (nan) atomicOr(&s_nan, 1);
        const double limb = (double)p.limb[(size_t)b * (size_t)p.limb_stride + c];
        for (int m = tid; m <= m_max; m += 256)
            if (fabs(sqrt((double)m) * step - limb) <= p.tol) { atomicMin(&s_lo, m); atomicMax(&s_hi, m); }
        __syncthreads();
        const bool none = s_hi < s_lo;                                           // no offset is allowed (or limb / tolerance is NaN)
        const int lo = none ? (1 << 30) : s_lo, hi = none ? -1 : s_hi;
        const unsigned span = none ? 0u : (unsigned)(hi - lo);
        double best = -INFINITY;
        int idx = RPSM_EMPTY;
        if (!s_nan) {
            int fd = RPSM_EMPTY;                                                 // the first disallowed child bin: the candidate 0.0
            for (int j = 0, jy = 0; jy < n && fd == RPSM_EMPTY; ++jy)
                for (int jx = 0; jx < n && fd == RPSM_EMPTY; ++jx)
                    for (int jz = 0; jz < n; ++jz, ++j) {
                        const int m = (iy - jy) * (iy - jy) + (ix - jx) * (ix - jx) + (iz - jz) * (iz - jz);
                        if ((unsigned)(m - lo) > span) { fd = j; break; }
                    }
            int j0 = 0;
            for (int jy = 0; jy < n; ++jy) {
                const int my = (iy - jy) * (iy - jy);
                for (int jx = 0; jx < n; ++jx, j0 += n) {
                    const int mxy = my + (ix - jx) * (ix - jx);
                    if (__builtin_amdgcn_ballot_w64(live && mxy <= hi) == 0) continue;       // out of every lane's reach
                    int jz = 0;                                                              // a row of n child bins, loads first
                    for (; jz + 8 <= n; jz += 8) rpsm_chunk<8>(se + j0 + jz, j0 + jz, iz - jz, mxy - lo, span, best, idx);
                    if (jz + 4 <= n) { rpsm_chunk<4>(se + j0 + jz, j0 + jz, iz - jz, mxy - lo, span, best, idx); jz += 4; }
                    for (; jz < n; ++jz) rpsm_chunk<1>(se + j0 + jz, j0 + jz, iz - jz, mxy - lo, span, best, idx);
                }
            }
            if (fd != RPSM_EMPTY && (idx == RPSM_EMPTY || 0.0 > best || (0.0 == best && fd < idx))) { best = 0.0; idx = fd; }
            if (idx == RPSM_EMPTY) { best = se[0]; idx = 0; }                    // every pair allowed and every energy -inf
        } else {
            int j = 0;
            for (int jy = 0; jy < n; ++jy)
                for (int jx = 0; jx < n; ++jx)
                    for (int jz = 0; jz < n; ++jz, ++j) {
                        const int m = (iy - jy) * (iy - jy) + (ix - jx) * (ix - jx) + (iz - jz) * (iz - jz);
                        const double val = (unsigned)(m - lo) <= span ? se[j] : 0.0;
                        if (idx == RPSM_EMPTY || (best == best && (val != val || val > best))) { best = val; idx = j; }
                    }
        }
        acc *= best;
        if (live) p.ws_back[((size_t)b * p.J + c) * (size_t)nb + i] = (unsigned short)idx;
    }
    if (live) eb[(size_t)node * nb + i] = acc;
}

__global__ __launch_bounds__(256) void rpsm_final_kernel(const RpsmParams p) {
    __shared__ double s_e[RPSM_MAX_J * RPSM_MAX_RBINS];          // a round's energies, [joint][bin]
    __shared__ unsigned char s_back[RPSM_MAX_J * RPSM_MAX_RBINS];
    __shared__ double s_pose[RPSM_MAX_J * 3];
    __shared__ int s_bin[RPSM_MAX_J];
    __shared__ double s_rv[4];
    __shared__ int s_ri[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, b = (int)blockIdx.x;
    const int J = p.J, nb = p.nb, rn = p.rn, rnb = p.rnb, root = p.tree.order[0];
    const double* eb = p.ws_energy + (size_t)b * J * (size_t)nb;
    const unsigned short* bb = p.ws_back + (size_t)b * J * (size_t)nb;
    int* bins = p.bins + (size_t)b * (size_t)(1 + p.depth) * J;

    // the root's first maximum
    double best = 0.0;
    int idx = RPSM_EMPTY;
    for (int j = tid; j < nb; j += 256) {
        const double e = eb[(size_t)root * nb + j];
        if (rpsm_ahead(e, j, best, idx)) { best = e; idx = j; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (rpsm_ahead(ov, oi, best, idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { s_rv[wave] = best; s_ri[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
        best = s_rv[0]; idx = s_ri[0];
        for (int k = 1; k < 4; ++k)
            if (rpsm_ahead(s_rv[k], s_ri[k], best, idx)) { best = s_rv[k]; idx = s_ri[k]; }
        p.energy[b] = best;
        s_bin[root] = idx;
        for (int k = 1; k < J; ++k) {                            // parents come before their children in `order`
            const int c = p.tree.order[k];
            const int q = bb[(size_t)c * nb + s_bin[p.tree.parent[c]]];
            s_bin[c] = q < nb ? q : nb - 1;
        }
    }
    __syncthreads();
    if (tid < J) {
        const double c[3] = {(double)p.root_center[(size_t)b * 3], (double)p.root_center[(size_t)b * 3 + 1], (double)p.root_center[(size_t)b * 3 + 2]};
        rpsm_point(s_bin[tid], p.n, p.grid_size, c, s_pose[tid * 3], s_pose[tid * 3 + 1], s_pose[tid * 3 + 2]);
        bins[tid] = s_bin[tid];
    }
    __syncthreads();

    double cur = p.grid_size / (double)p.n;
    for (int r = 0; r < p.depth; ++r) {
        for (int item = tid; item < J * rnb; item += 256) {      // unary on each joint's own grid
            const int j = item / rnb, q = item % rnb;
            double X, Y, Z, acc = 0.0;
            rpsm_point(q, rn, cur, s_pose + j * 3, X, Y, Z);
            for (int v = 0; v < p.V; ++v) {
                double ux, uy;
                if (rpsm_project(p, b, v, X, Y, Z, ux, uy)) acc += rpsm_sample(p.map(b, v, j), p.dtype, p.H, p.W, ux, uy);
            }
            s_e[j * RPSM_MAX_RBINS + q] = acc;
        }
        __syncthreads();
        for (int lev = p.tree.n_levels - 2; lev >= 0; --lev) {   // parents of depth lev, their children are complete
            const int first = p.tree.level_start[lev], cnt = p.tree.level_start[lev + 1] - first;
            for (int item = tid; item < cnt * rnb; item += 256) {
                const int node = p.tree.order[first + item / rnb], i = item % rnb;
                const int c_begin = p.tree.child_start[node], c_end = p.tree.child_start[node + 1];
                if (c_begin == c_end) continue;
                double PX, PY, PZ, acc = s_e[node * RPSM_MAX_RBINS + i];
                rpsm_point(i, rn, cur, s_pose + node * 3, PX, PY, PZ);
                for (int ci = c_begin; ci < c_end; ++ci) {
                    const int c = p.tree.child[ci];
                    const double limb = (double)p.limb[(size_t)b * (size_t)p.limb_stride + c];
                    double bv = 0.0;
                    int bi = RPSM_EMPTY;
                    for (int j = 0; j < rnb; ++j) {
                        double QX, QY, QZ;
                        rpsm_point(j, rn, cur, s_pose + c * 3, QX, QY, QZ);
                        const double dx = PX - QX, dy = PY - QY, dz = PZ - QZ;
                        const double d = sqrt(dx * dx + dy * dy + dz * dz);
                        const double val = fabs(d - limb) <= p.tol ? s_e[c * RPSM_MAX_RBINS + j] : 0.0;
                        if (bi == RPSM_EMPTY || (bv == bv && (val != val || val > bv))) { bv = val; bi = j; }
                    }
                    acc *= bv;
                    s_back[c * RPSM_MAX_RBINS + i] = (unsigned char)bi;
                }
                s_e[node * RPSM_MAX_RBINS + i] = acc;
            }
            __syncthreads();
        }
        if (tid == 0) {
            double bv = 0.0;
            int bi = RPSM_EMPTY;
            for (int j = 0; j < rnb; ++j) {
                const double val = s_e[root * RPSM_MAX_RBINS + j];
                if (bi == RPSM_EMPTY || (bv == bv && (val != val || val > bv))) { bv = val; bi = j; }
            }
            s_bin[root] = bi;
            for (int k = 1; k < J; ++k) {
                const int c = p.tree.order[k];
                s_bin[c] = s_back[c * RPSM_MAX_RBINS + s_bin[p.tree.parent[c]]];
            }
        }
        __syncthreads();
        if (tid < J) {                                           // a joint's grid hangs on its own point only
            double X, Y, Z;
            rpsm_point(s_bin[tid], rn, cur, s_pose + tid * 3, X, Y, Z);
            s_pose[tid * 3] = X; s_pose[tid * 3 + 1] = Y; s_pose[tid * 3 + 2] = Z;
            bins[(size_t)(r + 1) * J + tid] = s_bin[tid];
        }
        __syncthreads();
        cur = cur / (double)rn;
    }
    if (tid < J * 3) p.poses[(size_t)b * J * 3 + tid] = (float)s_pose[tid];
}

size_t rpsm_workspace_bytes(int B, int J, int first_nbins) {
    if (B <= 0 || B > (1 << 20) || J <= 0 || J > RPSM_MAX_J || first_nbins < 2 || first_nbins > 16) return 0;
    const size_t cells = (size_t)B * J * first_nbins * first_nbins * first_nbins;
    return cells * sizeof(double) + cells * sizeof(unsigned short);
}

// parents -> the tree tables; false unless it is one tree with exactly one root
static bool rpsm_build_tree(const int* parents, int J, RpsmTree& t) {
    int depth[RPSM_MAX_J], roots = 0;
    for (int j = 0; j < J; ++j) {
        if (parents[j] == -1) ++roots;
        else if (parents[j] < 0 || parents[j] >= J || parents[j] == j) return false;
    }
    if (roots != 1) return false;
    int max_depth = 0;
    for (int j = 0; j < J; ++j) {
        int d = 0, k = j;
        while (parents[k] != -1) {
            k = parents[k];
            if (++d >= J) return false;                          // a cycle
        }
        depth[j] = d;
        if (d > max_depth) max_depth = d;
    }
    t.n_levels = max_depth + 1;
    int at = 0;
    for (int d = 0; d <= max_depth; ++d) {
        t.level_start[d] = (unsigned char)at;
        for (int j = 0; j < J; ++j)
            if (depth[j] == d) t.order[at++] = (unsigned char)j;
    }
    for (int d = max_depth + 1; d <= RPSM_MAX_J; ++d) t.level_start[d] = (unsigned char)at;
    at = 0;
    for (int j = 0; j < J; ++j) {
        t.parent[j] = (signed char)parents[j];
        t.child_start[j] = (unsigned char)at;
        for (int c = 0; c < J; ++c)
            if (parents[c] == j) t.child[at++] = (unsigned char)c;
    }
    for (int j = J; j <= RPSM_MAX_J; ++j) t.child_start[j] = (unsigned char)at;
    return true;
}

int launch_rpsm(const void* const* heatmaps, int dtype, long long batch_stride, int B, int V, int J, int H, int W, const float* center,
                const float* scale, const double* cams_dev, const double* dist_dev, double img_w, double img_h, const float* root_center,
                const float* limb, long long limb_stride, const int* parents, int first_nbins, int recur_nbins, int recur_depth,
                double grid_size, double tolerance, void* workspace, size_t workspace_bytes, float* poses, int* bins, double* energy,
                int stages, hipStream_t s) {
    if (!center || !scale || !cams_dev || !root_center || !limb || !parents || !poses || !bins || !energy) return MPL_E_INVALID;
    if (B <= 0 || V <= 0 || J <= 0 || H <= 0 || W <= 0) return MPL_E_INVALID;
    if (!(img_w > 0) || !(img_h > 0) || !(grid_size > 0) || !(tolerance >= 0)) return MPL_E_INVALID;
    if (limb_stride != 0 && limb_stride < J) return MPL_E_INVALID;
    if (stages < 1 || stages > MPL_RPSM_ALL) return MPL_E_INVALID;
    RpsmParams p;
    if (const int rc = heatmap_table_fill(p, heatmaps, dtype, batch_stride, B, V, J, H, W)) return rc;
    if (J > RPSM_MAX_J || H < 2 || W < 2) return MPL_E_UNSUPPORTED;
    if (first_nbins < 2 || first_nbins > 16 || recur_nbins < 2 || recur_nbins > 4 || recur_depth < 0 || recur_depth > 16) return MPL_E_UNSUPPORTED;
    if (B > (1 << 20)) return MPL_E_UNSUPPORTED;
    if (!rpsm_build_tree(parents, J, p.tree)) return MPL_E_INVALID;
    if (!workspace || workspace_bytes < rpsm_workspace_bytes(B, J, first_nbins)) return MPL_E_WORKSPACE;
    p.center = center; p.scale = scale; p.cams = cams_dev; p.dist = dist_dev; p.root_center = root_center; p.limb = limb;
    p.limb_stride = limb_stride; p.poses = poses; p.bins = bins; p.energy = energy;
    p.n = first_nbins; p.nb = first_nbins * first_nbins * first_nbins; p.rn = recur_nbins; p.rnb = recur_nbins * recur_nbins * recur_nbins;
    p.depth = recur_depth; p.img_w = img_w; p.img_h = img_h; p.grid_size = grid_size; p.tol = tolerance;
    p.ws_energy = static_cast<double*>(workspace);
    p.ws_back = reinterpret_cast<unsigned short*>(p.ws_energy + (size_t)B * J * p.nb);
    const unsigned nblk = (unsigned)((p.nb + 255) / 256);
    if (stages & MPL_RPSM_UNARY) {
        ProfScope prof(MPL_K_FUSE_HEAD, s);
        hipLaunchKernelGGL(rpsm_unary_kernel, dim3(nblk * (unsigned)((J + RPSM_JG - 1) / RPSM_JG) * (unsigned)B), dim3(256), 0, s, p);
    }
    for (int lev = p.tree.n_levels - 2; lev >= 0 && (stages & MPL_RPSM_LEVELS); --lev) {
        const unsigned cnt = (unsigned)(p.tree.level_start[lev + 1] - p.tree.level_start[lev]);
        ProfScope prof(MPL_K_FUSE_HEAD, s);
        hipLaunchKernelGGL(rpsm_level_kernel, dim3(nblk * cnt * (unsigned)B), dim3(256), 0, s, p, lev);
    }
    if (stages & MPL_RPSM_FINAL) {
        ProfScope prof(MPL_K_FUSE_HEAD, s);
        hipLaunchKernelGGL(rpsm_final_kernel, dim3((unsigned)B), dim3(256), 0, s, p);
    }
    return hip_check_launch();
}

}  // namespace mpl
