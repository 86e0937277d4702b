// Procrustes alignment of a batch of predicted poses onto their targets: the transform behind PA-MPJPE (Protocol 2).
//
// Reference (MPL/lib/): utils/pose_utils.py:61-143 PoseUtils.procrustes, a numpy port of MATLAB's procrustes that runs one 3x3 SVD
// per pose on the host.  Row-vector convention as there: Z = scale * B @ R + translation, A the target, B the prediction.
//
// One work item = one pose, 64 poses per workgroup, every tensor read straight from global memory (a pose is 12 J contiguous
// bytes; its three passes after the first come from the cache).  Arithmetic is fp64 on the fp32 inputs and rounded once into the
// fp32 outputs.  No atomics, a fixed order of every sum: two runs give identical bits, and a pose does not depend on its batch.
//
// The SVD is a one-sided Jacobi (Hestenes) on M = A0n^T B0n itself: plane rotations from the right make the columns of M
// orthogonal, M V = W, so the singular values are the column norms of W and U its normalised columns.  Working on M rather than on
// M^T M keeps the small singular values to their own relative accuracy.  A fixed number of sweeps, unrolled, on named registers:
// no local array is indexed dynamically, so nothing lives in scratch.
#include "common.hpp"
#include "hestenes.hpp"

namespace mpl {

namespace {

constexpr int PROC_POSES = 64;        // poses (= work items) of one workgroup
constexpr int PROC_SWEEPS = 6;        // cyclic sweeps over the column pairs (0,1) (0,2) (1,2); at fp64 round-off after 4 (numpy simulation)
constexpr double PROC_RANK_TOL = 1e-12;

struct ProcArgs {
    const float* pred;
    const float* target;
    const float* conf;          // (B,J) or NULL
    float* aligned;             // (B,J,3) or NULL
    float* d;                   // (B) or NULL
    float* rotation;            // (B,3,3) or NULL
    float* scale;               // (B) or NULL
    float* translation;         // (B,3) or NULL
    float sc[3], of[3];         // de-normalisation on load, both tensors
    int B, J;
    int n;                      // joints listed for participation: n_sel, or J without a selection
    int has_sel, scaling, reflection;
    unsigned char sel[64];
};

__device__ __forceinline__ bool proc_takes_part(const ProcArgs& p, size_t b, int j) {
    return !p.conf || takes_part((double)p.conf[b * p.J + j]);
}

// one Hestenes rotation: columns a and b of M (and of V) are turned so that a . b = 0
__device__ __forceinline__ void proc_rotate(double& a0, double& a1, double& a2, double& b0, double& b1, double& b2, double& va0,
                                            double& va1, double& va2, double& vb0, double& vb1, double& vb2) {
    const double alpha = a0 * a0 + a1 * a1 + a2 * a2, beta = b0 * b0 + b1 * b1 + b2 * b2, gamma = a0 * b0 + a1 * b1 + a2 * b2;
    const Rotation rot = hestenes_rotation(alpha, beta, gamma);
    const double c = rot.cs, s = rot.sn;
    double x;
    x = a0; a0 = c * x - s * b0; b0 = s * x + c * b0;
    x = a1; a1 = c * x - s * b1; b1 = s * x + c * b1;
    x = a2; a2 = c * x - s * b2; b2 = s * x + c * b2;
    x = va0; va0 = c * x - s * vb0; vb0 = s * x + c * vb0;
    x = va1; va1 = c * x - s * vb1; vb1 = s * x + c * vb1;
    x = va2; va2 = c * x - s * vb2; vb2 = s * x + c * vb2;
}

__device__ __forceinline__ void proc_swap(double& x, double& y) {
    const double t = x;
    x = y;
    y = t;
}

__global__ __launch_bounds__(PROC_POSES) void procrustes_align_kernel(const ProcArgs p) {
    const long long idx = (long long)blockIdx.x * PROC_POSES + threadIdx.x;
    if (idx >= p.B) return;
    const size_t b = (size_t)idx;
    const float* A = p.target + b * p.J * 3;
    const float* Bp = p.pred + b * p.J * 3;
    const double sx = (double)p.sc[0], sy = (double)p.sc[1], sz = (double)p.sc[2];
    const double ox = (double)p.of[0], oy = (double)p.of[1], oz = (double)p.of[2];

    // pass 1: the means over the joints that take part
    double am0 = 0, am1 = 0, am2 = 0, bm0 = 0, bm1 = 0, bm2 = 0;
    int cnt = 0;
    for (int k = 0; k < p.n; ++k) {
        const int j = p.has_sel ? (int)p.sel[k] : k;
        if (!proc_takes_part(p, b, j)) continue;
        am0 += (double)A[j * 3 + 0] * sx + ox;
        am1 += (double)A[j * 3 + 1] * sy + oy;
        am2 += (double)A[j * 3 + 2] * sz + oz;
        bm0 += (double)Bp[j * 3 + 0] * sx + ox;
        bm1 += (double)Bp[j * 3 + 1] * sy + oy;
        bm2 += (double)Bp[j * 3 + 2] * sz + oz;
        ++cnt;
    }
    const double inv_n = 1.0 / (double)(cnt > 0 ? cnt : 1);
    am0 *= inv_n; am1 *= inv_n; am2 *= inv_n;
    bm0 *= inv_n; bm1 *= inv_n; bm2 *= inv_n;

    // pass 2: ssX, ssY and A0^T B0 of the centred points (m_rc: row r of A0^T, column c of B0)
    double ssX = 0, ssY = 0;
    double m00 = 0, m01 = 0, m02 = 0, m10 = 0, m11 = 0, m12 = 0, m20 = 0, m21 = 0, m22 = 0;
    for (int k = 0; k < p.n; ++k) {
        const int j = p.has_sel ? (int)p.sel[k] : k;
        if (!proc_takes_part(p, b, j)) continue;
        const double a0 = (double)A[j * 3 + 0] * sx + ox - am0, a1 = (double)A[j * 3 + 1] * sy + oy - am1,
                     a2 = (double)A[j * 3 + 2] * sz + oz - am2;
        const double b0 = (double)Bp[j * 3 + 0] * sx + ox - bm0, b1 = (double)Bp[j * 3 + 1] * sy + oy - bm1,
                     b2 = (double)Bp[j * 3 + 2] * sz + oz - bm2;
        ssX += a0 * a0 + a1 * a1 + a2 * a2;
        ssY += b0 * b0 + b1 * b1 + b2 * b2;
        m00 += a0 * b0; m01 += a0 * b1; m02 += a0 * b2;
        m10 += a1 * b0; m11 += a1 * b1; m12 += a1 * b2;
        m20 += a2 * b0; m21 += a2 * b1; m22 += a2 * b2;
    }
    // degenerate input (a statement about the pose, not a device error): fewer than 3 joints, a zero or non-finite spread
    bool bad = cnt < 3 || !(ssX > 0.0 && ssX <= FINITE_MAX) || !(ssY > 0.0 && ssY <= FINITE_MAX);
    const double a_norm = sqrt(ssX), b_norm = sqrt(ssY);
    const double inv_ab = 1.0 / (a_norm * b_norm);
    m00 *= inv_ab; m01 *= inv_ab; m02 *= inv_ab;
    m10 *= inv_ab; m11 *= inv_ab; m12 *= inv_ab;
    m20 *= inv_ab; m21 *= inv_ab; m22 *= inv_ab;

    // M = U diag(s) V^T: the columns of M become W = U diag(s), V collects the rotations (v_rc)
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#pragma unroll
    for (int sweep = 0; sweep < PROC_SWEEPS; ++sweep) {
        proc_rotate(m00, m10, m20, m01, m11, m21, v00, v10, v20, v01, v11, v21);
        proc_rotate(m00, m10, m20, m02, m12, m22, v00, v10, v20, v02, v12, v22);
        proc_rotate(m01, m11, m21, m02, m12, m22, v01, v11, v21, v02, v12, v22);
    }
    double s0 = sqrt(m00 * m00 + m10 * m10 + m20 * m20), s1 = sqrt(m01 * m01 + m11 * m11 + m21 * m21),
           s2 = sqrt(m02 * m02 + m12 * m12 + m22 * m22);
    // descending order, so that "the last column" is the one numpy means (a swap of the same columns of W and V leaves V U^T alone)
    if (s0 < s1) {
        proc_swap(s0, s1);
        proc_swap(m00, m01); proc_swap(m10, m11); proc_swap(m20, m21);
        proc_swap(v00, v01); proc_swap(v10, v11); proc_swap(v20, v21);
    }
    if (s1 < s2) {
        proc_swap(s1, s2);
        proc_swap(m01, m02); proc_swap(m11, m12); proc_swap(m21, m22);
        proc_swap(v01, v02); proc_swap(v11, v12); proc_swap(v21, v22);
    }
    if (s0 < s1) {
        proc_swap(s0, s1);
        proc_swap(m00, m01); proc_swap(m10, m11); proc_swap(m20, m21);
        proc_swap(v00, v01); proc_swap(v10, v11); proc_swap(v20, v21);
    }
    bad = bad || !(s1 > PROC_RANK_TOL * s0);          // collinear points (or NaN): the rotation is not determined
    // U = W diag(1 / s)
    const double i0 = 1.0 / s0, i1 = 1.0 / s1;
    const double u00 = m00 * i0, u10 = m10 * i0, u20 = m20 * i0;
    const double u01 = m01 * i1, u11 = m11 * i1, u21 = m21 * i1;
    // the third left vector is +-(u0 x u1), the sign that of its own column of W: a small s[2] costs it no accuracy
    double u02 = u10 * u21 - u20 * u11, u12 = u20 * u01 - u00 * u21, u22 = u00 * u11 - u10 * u01;
    if (s2 > PROC_RANK_TOL * s0) {
        if (u02 * m02 + u12 * m12 + u22 * m22 < 0.0) {
            u02 = -u02; u12 = -u12; u22 = -u22;
        }
    } else {
        // coplanar points: both signs of the third pair fit equally well; U and V are completed by cross products, which makes
        // both proper and R = V U^T the proper rotation (the documented deviation from numpy's arbitrary sign)
        v02 = v10 * v21 - v20 * v11; v12 = v20 * v01 - v00 * v21; v22 = v00 * v11 - v10 * v01;
    }
    // det(V U^T) = det V det U decides the reflection modes (pose_utils.py:111-119)
    const double det_u = u00 * (u11 * u22 - u12 * u21) - u01 * (u10 * u22 - u12 * u20) + u02 * (u10 * u21 - u11 * u20);
    const double det_v = v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20) + v02 * (v10 * v21 - v11 * v20);
    const double det_r = det_u * det_v;
    double sg = 1.0;        // -1: the last column of V and s[2] change sign
    if (p.reflection == 1 && det_r < 0.0) sg = -1.0;
    if (p.reflection == 2 && det_r > 0.0) sg = -1.0;
    // R = V U^T: r_ik = sum_c v_ic u_kc
    const double r00 = v00 * u00 + v01 * u01 + sg * v02 * u02, r01 = v00 * u10 + v01 * u11 + sg * v02 * u12,
                 r02 = v00 * u20 + v01 * u21 + sg * v02 * u22;
    const double r10 = v10 * u00 + v11 * u01 + sg * v12 * u02, r11 = v10 * u10 + v11 * u11 + sg * v12 * u12,
                 r12 = v10 * u20 + v11 * u21 + sg * v12 * u22;
    const double r20 = v20 * u00 + v21 * u01 + sg * v22 * u02, r21 = v20 * u10 + v21 * u11 + sg * v22 * u12,
                 r22 = v20 * u20 + v21 * u21 + sg * v22 * u22;
    const double S = s0 + s1 + sg * s2;
    const double g = p.scaling ? S * a_norm / b_norm : 1.0;       // Z = g (B - B_bar) R + A_bar in both modes (B0 = B_norm B0n)

    float* Z = p.aligned ? p.aligned + b * p.J * 3 : nullptr;
    if (bad) {
        const float nan = __builtin_nanf("");
        if (Z)
            for (int e = 0; e < p.J * 3; ++e) Z[e] = nan;
        if (p.d) p.d[b] = nan;
        if (p.scale) p.scale[b] = nan;
        if (p.rotation)
            for (int e = 0; e < 9; ++e) p.rotation[b * 9 + e] = nan;
        if (p.translation) p.translation[b * 3 + 0] = p.translation[b * 3 + 1] = p.translation[b * 3 + 2] = nan;
        return;
    }
    if (p.rotation) {
        float* R = p.rotation + b * 9;
        R[0] = (float)r00; R[1] = (float)r01; R[2] = (float)r02;
        R[3] = (float)r10; R[4] = (float)r11; R[5] = (float)r12;
        R[6] = (float)r20; R[7] = (float)r21; R[8] = (float)r22;
    }
    if (p.scale) p.scale[b] = (float)g;
    if (p.translation) {
        p.translation[b * 3 + 0] = (float)(am0 - g * (bm0 * r00 + bm1 * r10 + bm2 * r20));
        p.translation[b * 3 + 1] = (float)(am1 - g * (bm0 * r01 + bm1 * r11 + bm2 * r21));
        p.translation[b * 3 + 2] = (float)(am2 - g * (bm0 * r02 + bm1 * r12 + bm2 * r22));
    }
    // pass 3: Z for every joint of the pose
    if (Z)
        for (int j = 0; j < p.J; ++j) {
            const double b0 = (double)Bp[j * 3 + 0] * sx + ox - bm0, b1 = (double)Bp[j * 3 + 1] * sy + oy - bm1,
                         b2 = (double)Bp[j * 3 + 2] * sz + oz - bm2;
            Z[j * 3 + 0] = (float)(g * (b0 * r00 + b1 * r10 + b2 * r20) + am0);
            Z[j * 3 + 1] = (float)(g * (b0 * r01 + b1 * r11 + b2 * r21) + am1);
            Z[j * 3 + 2] = (float)(g * (b0 * r02 + b1 * r12 + b2 * r22) + am2);
        }
    // the residual on the points themselves, over the joints that took part: 1 - S^2 cancels to nothing where the fit is good
    if (p.d) {
        double res = 0;
        for (int k = 0; k < p.n; ++k) {
            const int j = p.has_sel ? (int)p.sel[k] : k;
            if (!proc_takes_part(p, b, j)) continue;
            const double b0 = (double)Bp[j * 3 + 0] * sx + ox - bm0, b1 = (double)Bp[j * 3 + 1] * sy + oy - bm1,
                         b2 = (double)Bp[j * 3 + 2] * sz + oz - bm2;
            const double e0 = g * (b0 * r00 + b1 * r10 + b2 * r20) - ((double)A[j * 3 + 0] * sx + ox - am0);
            const double e1 = g * (b0 * r01 + b1 * r11 + b2 * r21) - ((double)A[j * 3 + 1] * sy + oy - am1);
            const double e2 = g * (b0 * r02 + b1 * r12 + b2 * r22) - ((double)A[j * 3 + 2] * sz + oz - am2);
            res += e0 * e0 + e1 * e1 + e2 * e2;
        }
        p.d[b] = (float)(res / ssX);
    }
}

}  // namespace

int launch_procrustes_align(const float* pred, const float* target, const float* conf, const int* sel, int n_sel, const float* scale3,
                            const float* offset3, int scaling, int reflection, int B, int J, float* aligned, float* d,
                            float* rotation, float* scale, float* translation, hipStream_t s) {
    if (!pred || !target || B <= 0 || J <= 0 || (sel && n_sel <= 0) || reflection < 0 || reflection > 2) return MPL_E_INVALID;
    if (!aligned && !d) return MPL_E_INVALID;
    if (J > 64 || (sel && n_sel > 64) || (long long)B * J > (1ll << 30)) return MPL_E_UNSUPPORTED;
    ProcArgs p;
    p.pred = pred; p.target = target; p.conf = conf;
    p.aligned = aligned; p.d = d; p.rotation = rotation; p.scale = scale; p.translation = translation;
    for (int k = 0; k < 3; ++k) {
        p.sc[k] = scale3 ? scale3[k] : 1.f;
        p.of[k] = offset3 ? offset3[k] : 0.f;
    }
    p.B = B; p.J = J;
    p.has_sel = sel != nullptr;
    p.n = sel ? n_sel : J;
    p.scaling = scaling != 0;
    p.reflection = reflection;
    for (int k = 0; k < 64; ++k) {
        p.sel[k] = 0;
        if (sel && k < n_sel) {
            if (sel[k] < 0 || sel[k] >= J) return MPL_E_INVALID;
            p.sel[k] = (unsigned char)sel[k];
        }
    }
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(procrustes_align_kernel, dim3((unsigned)((B + PROC_POSES - 1) / PROC_POSES)), dim3(PROC_POSES), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
