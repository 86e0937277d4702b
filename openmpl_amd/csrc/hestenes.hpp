// The one-sided Jacobi (Hestenes) of the pose utilities, stated once for the device and for a host build: the plane rotation that
// makes two columns orthogonal, its use on a 3 x 3 in registers, the 3 x 3 factorisation by fixed sweeps, and the lane-interleaved
// addressing of what a solver indexes by a loop counter.  procrustes.hip takes the rotation alone (its 3 x 3 lives in named
// registers and is sorted afterwards); locate_cameras.hip and five_point.hpp take all of it.  The two column sweeps (12 columns
// over 24 rows there, 9 over 14 here) stay with their files: they share the rotation, and each keeps its own threshold and exit
// (DESIGN.md section 7).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MPL_HD __host__ __device__ __forceinline__
#else
#define MPL_HD inline
#endif

namespace mpl {

constexpr int SWEEPS3 = 6;               // cyclic sweeps of a 3 x 3 over the pairs (0,1) (0,2) (1,2): fixed, as in procrustes.hip

// element e of a lane's storage at p[e * S]: S = 64 on the device, where the doubles of the 64 lanes of a wave are interleaved in
// LDS (64 lanes read 512 contiguous bytes, no bank conflict), S = 1 in a host build
template <int S>
struct Strided {
    double* p;
    MPL_HD double& operator[](int e) const { return p[e * S]; }
};

// The rotation (cs, sn) under which columns a and b, with alpha = a . a, beta = b . b, gamma = a . b, become
// a' = cs a - sn b, b' = sn a + cs b with a' . b' = 0.  gamma = 0 (and |zeta| = inf): the identity.  Whether a pair is turned at
// all is the caller's to say; NONZERO: it has seen that gamma != 0 (its threshold says so), and the question is not asked again --
// in the sweep of locate_cameras.hip the second test cost two registers of the scoring loop their place
struct Rotation {
    double cs, sn;
};

template <bool NONZERO = false>
MPL_HD Rotation hestenes_rotation(double alpha, double beta, double gamma) {
    double t = 0.0;
    if (NONZERO || gamma != 0.0) {
        const double zeta = (beta - alpha) / (2.0 * gamma);
        t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    }
    const double cs = 1.0 / sqrt(1.0 + t * t);
    return Rotation{cs, cs * t};
}

// one rotation of a 3 x 3: columns a and b of M (and of W) are turned so that a . b = 0
MPL_HD void rotate3(double (&M)[3][3], double (&W)[3][3], const int a, const int b) {
    const double alpha = M[0][a] * M[0][a] + M[1][a] * M[1][a] + M[2][a] * M[2][a];
    const double beta = M[0][b] * M[0][b] + M[1][b] * M[1][b] + M[2][b] * M[2][b];
    const double gamma = M[0][a] * M[0][b] + M[1][a] * M[1][b] + M[2][a] * M[2][b];
    const Rotation rot = hestenes_rotation(alpha, beta, gamma);
    const double cs = rot.cs, sn = rot.sn;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double x = M[r][a];
        M[r][a] = cs * x - sn * M[r][b];
        M[r][b] = sn * x + cs * M[r][b];
        x = W[r][a];
        W[r][a] = cs * x - sn * W[r][b];
        W[r][b] = sn * x + cs * W[r][b];
    }
}

// M = U S W^T by SWEEPS3 sweeps: M becomes U S (orthogonal columns), W collects the rotations from the identity, sv holds the
// column norms -> the shortest column, the lowest among equals
MPL_HD int factor3(double (&M)[3][3], double (&W)[3][3], double (&sv)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) W[r][c] = r == c ? 1.0 : 0.0;
    }
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS3; ++sweep) {
        rotate3(M, W, 0, 1);
        rotate3(M, W, 0, 2);
        rotate3(M, W, 1, 2);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sv[k] = sqrt(M[0][k] * M[0][k] + M[1][k] * M[1][k] + M[2][k] * M[2][k]);
    return (sv[2] <= sv[0] && sv[2] <= sv[1]) ? 2 : (sv[1] <= sv[0] ? 1 : 0);
}

}  // namespace mpl
