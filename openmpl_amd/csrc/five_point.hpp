// The five-point relative pose solver of relative_pose.hip, stated once for the device and for a host build: from five
// correspondences y_b^T E y_a = 0 in normalised coordinates to at most ten essential matrices, and from an essential matrix to the
// pose (R, t) with x_b = R x_a + t, |t| = 1.  include/mpl_hip.h (mpl_relative_pose, step 3) states the arithmetic;
// tests/relative_pose_cases.py restates it in numpy.
//
// Nister's route (An efficient solution to the five-point relative pose problem, PAMI 2004): the null space of the 5 x 9 system is
// E = x X + y Y + z Z + W; det E = 0 and 2 E E^T E - tr(E E^T) E = 0 are ten cubics in (x, y, z); Gauss-Jordan elimination on the
// ten monomials that hold x or y to the second power or more leaves rows in x [z^2], y [z^2], 1 [z^3]; three differences
// <x^2 z> - z <x^2>, <y^2 z> - z <y^2>, <xyz> - z <xy> form a 3 x 3 polynomial matrix B(z) with B(z) (x, y, 1)^T = 0, whose
// determinant has degree 10.  Its real roots are isolated by a Sturm chain, bisected and polished by Newton: no complex arithmetic.
// Added to that route: a basis of the null space that does not depend on how it was found (canonical_basis), and a polish of every
// (x, y, z) on the ten cubics (polish).
//
// Storage: what is indexed by a loop counter (the 14 x 9 stacked system of the Jacobi, the 10 x 20 elimination, the Sturm chain)
// goes through Strided<S> of hestenes.hpp -- S = 64 on the device, where the FP_DOUBLES doubles of a lane are interleaved in LDS,
// S = 1 in a host build.  Everything else has constant indices after unrolling and lives in registers.  The rotation of the Jacobi
// and the 3 x 3 factorisation of pose_of are those of hestenes.hpp.
#pragma once
#include "hestenes.hpp"

// the value as it is, but nothing the compiler knows about it
#if defined(__HIP_DEVICE_COMPILE__)
#define MPL_FP_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define MPL_FP_OPAQUE(x) asm volatile("" : "+m"(x))
#endif

namespace mpl {
namespace fivept {

constexpr int FP_SAMPLE = 5;
constexpr int FP_ROWS = 14;              // a column of the stacked [A; V]: 5 rows of the system over 9 of the rotations
constexpr int FP_DOUBLES = 249;          // of a lane: the 10 x 20 cubics (the largest of the three uses), the ten roots and B(z) beside them
constexpr int FP_SWEEPS = 30;            // a cap of the 9-column Jacobi
constexpr double FP_ROT_EPS = 1e-15;     // columns with |a . b| <= this * |A|_F^2 are not turned
constexpr int FP_MAX_ROOTS = 10, FP_ROOTS_AT = 200, FP_BZ_AT = 210;
constexpr int FP_POLISH = 3;             // Gauss-Newton steps of a candidate on the ten cubics: fixed
constexpr double FP_TRIM = 1e-13;        // a leading coefficient below this times the largest is no coefficient
constexpr int FP_ISOLATE = 64, FP_BISECT = 80, FP_NEWTON = 3;
constexpr double FP_DEPTH_MIN = 1e-9;    // CAMERA_Z_MIN of views.hpp: a sample at a depth <= this is not in front

// ---- polynomials in (x, y, z).  Degree 1: x y z 1.  Degree 2: x^2 xy xz y^2 yz z^2 x y z 1.  Degree 3, the columns of the
// elimination: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | x xz xz^2 y yz yz^2 1 z z^2 z^3
MPL_HD constexpr int exp1(int i, int v) { return i == v ? 1 : 0; }
MPL_HD constexpr int exp2(int i, int v) {
    return v == 0 ? (i == 0 ? 2 : (i == 1 || i == 2 || i == 6) ? 1 : 0)
         : v == 1 ? (i == 3 ? 2 : (i == 1 || i == 4 || i == 7) ? 1 : 0)
                  : (i == 5 ? 2 : (i == 2 || i == 4 || i == 8) ? 1 : 0);
}
MPL_HD constexpr int slot2(int a, int b, int c) {
    return a == 2 ? 0 : b == 2 ? 3 : c == 2 ? 5 : (a == 1 && b == 1) ? 1 : (a == 1 && c == 1) ? 2 : (b == 1 && c == 1) ? 4
         : a == 1 ? 6 : b == 1 ? 7 : c == 1 ? 8 : 9;
}
MPL_HD constexpr int slot3(int a, int b, int c) {
    return a == 3 ? 0 : b == 3 ? 1 : (a == 2 && b == 1) ? 2 : (a == 1 && b == 2) ? 3 : (a == 2 && c == 1) ? 4 : a == 2 ? 5
         : (b == 2 && c == 1) ? 6 : b == 2 ? 7 : (a == 1 && b == 1 && c == 1) ? 8 : (a == 1 && b == 1) ? 9
         : a == 1 ? 10 + c : b == 1 ? 13 + c : 16 + c;
}

// out2 += sign * a * b, a and b of degree 1
MPL_HD void mul11(const double (&a)[4], const double (&b)[4], double sign, double (&out)[10]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            out[slot2(exp1(i, 0) + exp1(j, 0), exp1(i, 1) + exp1(j, 1), exp1(i, 2) + exp1(j, 2))] += sign * (a[i] * b[j]);
    }
}

// out3 += sign * a * b, a of degree 2 and b of degree 1
MPL_HD void mul21(const double (&a)[10], const double (&b)[4], double sign, double (&out)[20]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            out[slot3(exp2(i, 0) + exp1(j, 0), exp2(i, 1) + exp1(j, 1), exp2(i, 2) + exp1(j, 2))] += sign * (a[i] * b[j]);
    }
}

// c += sign * a * b for polynomials in z, coefficients ascending
template <int NA, int NB>
MPL_HD void mulz(const double (&a)[NA], const double (&b)[NB], double sign, double (&c)[NA + NB - 1]) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
#pragma unroll
        for (int j = 0; j < NB; ++j) c[i + j] += sign * (a[i] * b[j]);
    }
}

// ---- An orthonormal basis N of the null space -> the basis that does not depend on which one it was: the projector N N^T is the
// same for all of them, and X, Y, Z, W are its columns at the four largest entries of its diagonal, in descending order (the lowest
// index among equals), made orthonormal in that order.  The roots (x, y, z) then belong to the five samples and not to the way the null space was found, so that two
// implementations meet the same near-coincident roots at the same hypotheses
MPL_HD void canonical_basis(double (&basis)[4][9]) {
    double diag[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) diag[e] = basis[0][e] * basis[0][e] + basis[1][e] * basis[1][e] + basis[2][e] * basis[2][e] + basis[3][e] * basis[3][e];
    double out[4][9];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int kmax = 0;
        double dmax = -1.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            if (diag[e] > dmax) {
                dmax = diag[e];
                kmax = e;
            }
        }
        double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            if (e == kmax) {
                diag[e] = -1.0;              // taken
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = basis[j][e];
            }
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) out[k][e] = c[0] * basis[0][e] + c[1] * basis[1][e] + c[2] * basis[2][e] + c[3] * basis[3][e];
    }
    // made orthonormal in that order, Gram-Schmidt with every projection taken twice: E = x X + y Y + z Z + W on a basis that is
    // not orthonormal loses digits where two of the four are close
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int j = 0; j < k; ++j) {
                double dot = 0.0;
#pragma unroll
                for (int e = 0; e < 9; ++e) dot += basis[j][e] * out[k][e];
#pragma unroll
                for (int e = 0; e < 9; ++e) out[k][e] -= dot * basis[j][e];
            }
        }
        double n2 = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) n2 += out[k][e] * out[k][e];
        const double inv = 1.0 / sqrt(n2);
#pragma unroll
        for (int e = 0; e < 9; ++e) basis[k][e] = out[k][e] * inv;
    }
}

// ---- the null space of the 5 x 9 system: rows kron(d_b, d_a) of the five samples, d = (y0, y1, 1), so that a row times vec(E)
// (row-major) is d_b^T E d_a.  One-sided Jacobi (Hestenes) on the system itself; the four shortest columns of A V carry the null
// space in the rows of V below them, the lowest column among equals first; canonical_basis makes X, Y, Z, W of them.  basis[k][e]:
// entry e of X, Y, Z, W
template <int S>
MPL_HD void null_space(Strided<S> m, const double (&ya)[FP_SAMPLE][2], const double (&yb)[FP_SAMPLE][2], double (&basis)[4][9]) {
    double frob = 0.0;
#pragma unroll
    for (int i = 0; i < FP_SAMPLE; ++i) {
        const double da[3] = {ya[i][0], ya[i][1], 1.0}, db[3] = {yb[i][0], yb[i][1], 1.0};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = db[r] * da[c];
                m[(3 * r + c) * FP_ROWS + i] = e;
                frob += e * e;
            }
        }
    }
    for (int col = 0; col < 9; ++col)
        for (int r = 0; r < 9; ++r) m[col * FP_ROWS + 5 + r] = r == col ? 1.0 : 0.0;
    for (int sweep = 0; sweep < FP_SWEEPS; ++sweep) {
        bool turned = false;
        for (int ca = 0; ca < 8; ++ca) {
            for (int cb = ca + 1; cb < 9; ++cb) {
                double a[FP_ROWS], b[FP_ROWS];
#pragma unroll
                for (int r = 0; r < FP_ROWS; ++r) {
                    a[r] = m[ca * FP_ROWS + r];
                    b[r] = m[cb * FP_ROWS + r];
                }
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    alpha += a[r] * a[r];
                    beta += b[r] * b[r];
                    gamma += a[r] * b[r];
                }
                // measured against |A|_F^2 and not against |a| |b|: four columns shrink to nothing, and relative to themselves they
                // would be turned against each other for ever
                if (fabs(gamma) > FP_ROT_EPS * frob) {
                    const Rotation rot = hestenes_rotation(alpha, beta, gamma);
                    const double cs = rot.cs, sn = rot.sn;
#pragma unroll
                    for (int r = 0; r < FP_ROWS; ++r) {
                        m[ca * FP_ROWS + r] = cs * a[r] - sn * b[r];
                        m[cb * FP_ROWS + r] = sn * a[r] + cs * b[r];
                    }
                    turned = true;
                }
            }
        }
        if (!turned) break;
    }
    double n2[9];
#pragma unroll
    for (int col = 0; col < 9; ++col) {
        n2[col] = 0.0;
#pragma unroll
        for (int r = 0; r < 5; ++r) n2[col] += m[col * FP_ROWS + r] * m[col * FP_ROWS + r];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int kmin = 0;
        double smin = __builtin_inf();
#pragma unroll
        for (int col = 0; col < 9; ++col) {
            if (n2[col] < smin) {
                smin = n2[col];
                kmin = col;
            }
        }
#pragma unroll
        for (int col = 0; col < 9; ++col) n2[col] = col == kmin ? __builtin_inf() : n2[col];     // taken
#pragma unroll
        for (int e = 0; e < 9; ++e) basis[k][e] = m[kmin * FP_ROWS + 5 + e];
    }
    canonical_basis(basis);
}

// ---- the ten cubics into the 10 x 20 matrix m (row-major, row r at m[20 r]): row 0 is det E, rows 1 .. 9 the entries of
// (E E^T - tr(E E^T) / 2) E, row-major
template <int S>
MPL_HD void constraints(Strided<S> m, const double (&basis)[4][9]) {
    double E[9][4];                          // entry e of E as a polynomial of degree 1
#pragma unroll
    for (int e = 0; e < 9; ++e) {
#pragma unroll
        for (int k = 0; k < 4; ++k) E[e][k] = basis[k][e];
    }
    {
        double det[20];
#pragma unroll
        for (int k = 0; k < 20; ++k) det[k] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {        // the expansion along row 0: E0c (E1,c+1 E2,c+2 - E1,c+2 E2,c+1), columns cyclic
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            double minor[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) minor[k] = 0.0;
            mul11(E[3 + c1], E[6 + c2], 1.0, minor);
            mul11(E[3 + c2], E[6 + c1], -1.0, minor);
            mul21(minor, E[c], 1.0, det);
        }
#pragma unroll
        for (int k = 0; k < 20; ++k) m[k] = det[k];
    }
    double G[3][3][10];                      // E E^T - tr / 2, symmetric: the upper triangle is formed, the lower copied
    double tr[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) tr[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) {
#pragma unroll
            for (int k = 0; k < 10; ++k) G[i][j][k] = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) mul11(E[3 * i + c], E[3 * j + c], 1.0, G[i][j]);
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) tr[k] += G[i][i][k];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 10; ++k) G[i][i][k] -= 0.5 * tr[k];
#pragma unroll
        for (int j = 0; j < i; ++j) {
#pragma unroll
            for (int k = 0; k < 10; ++k) G[i][j][k] = G[j][i][k];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double row[20];
#pragma unroll
            for (int k = 0; k < 20; ++k) row[k] = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) mul21(G[i][c], E[3 * c + j], 1.0, row);
#pragma unroll
            for (int k = 0; k < 20; ++k) m[(1 + 3 * i + j) * 20 + k] = row[k];
        }
    }
}

// ---- Gauss-Jordan elimination of the first ten columns with partial pivoting (the lowest row among equals) -> [I | B]; false:
// a pivot that is zero or not a number
template <int S>
MPL_HD bool eliminate(Strided<S> m) {
    for (int k = 0; k < 10; ++k) {
        int piv = k;
        double best = fabs(m[k * 20 + k]);
        for (int r = k + 1; r < 10; ++r) {
            const double v = fabs(m[r * 20 + k]);
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        if (!(best > 0.0) || !(best <= 1.79769313486231570815e308)) return false;
        const double inv = 1.0 / m[piv * 20 + k];
        for (int c = k; c < 20; ++c) {       // the pivot row, scaled, changes places with row k
            const double v = m[piv * 20 + c] * inv;
            m[piv * 20 + c] = m[k * 20 + c];
            m[k * 20 + c] = v;
        }
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = m[r * 20 + k];
            for (int c = k; c < 20; ++c) m[r * 20 + c] -= f * m[k * 20 + c];
        }
    }
    return true;
}

// ---- B(z): row r holds the polynomials of x (4), y (4) and 1 (5), ascending, of <lead z> - z <lead>, for the rows 4 / 5 (x^2 z,
// x^2), 6 / 7 (y^2 z, y^2) and 8 / 9 (xyz, xy) of the eliminated matrix
template <int S>
MPL_HD void hidden_variable(Strided<S> m, double (&Bz)[3][13]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int e = (4 + 2 * r) * 20, f = (5 + 2 * r) * 20;
#pragma unroll
        for (int g = 0; g < 2; ++g) {        // the x group at columns 10 .. 12, the y group at 13 .. 15
            const int c0 = 10 + 3 * g;
            Bz[r][4 * g + 0] = m[e + c0];
            Bz[r][4 * g + 1] = m[e + c0 + 1] - m[f + c0];
            Bz[r][4 * g + 2] = m[e + c0 + 2] - m[f + c0 + 1];
            Bz[r][4 * g + 3] = -m[f + c0 + 2];
        }
        Bz[r][8] = m[e + 16];
        Bz[r][9] = m[e + 17] - m[f + 16];
        Bz[r][10] = m[e + 18] - m[f + 17];
        Bz[r][11] = m[e + 19] - m[f + 18];
        Bz[r][12] = -m[f + 19];
    }
}

// det B(z), degree 10, ascending
MPL_HD void determinant(const double (&Bz)[3][13], double (&p)[11]) {
    double a[3][4], b[3][4], c[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[r][k] = Bz[r][k];
            b[r][k] = Bz[r][4 + k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) c[r][k] = Bz[r][8 + k];
    }
#pragma unroll
    for (int k = 0; k < 11; ++k) p[k] = 0.0;
    double bc[8], ac[8], ab[7];
#pragma unroll
    for (int k = 0; k < 8; ++k) bc[k] = ac[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) ab[k] = 0.0;
    mulz(b[1], c[2], 1.0, bc);
    mulz(b[2], c[1], -1.0, bc);
    mulz(a[1], c[2], 1.0, ac);
    mulz(a[2], c[1], -1.0, ac);
    mulz(a[1], b[2], 1.0, ab);
    mulz(a[2], b[1], -1.0, ab);
    mulz(a[0], bc, 1.0, p);
    mulz(b[0], ac, -1.0, p);
    mulz(c[0], ab, 1.0, p);
}

// ---- the real roots of p (degree <= 10, ascending) in ascending order -> their number.  m: the lane's storage; the chain's
// polynomial k is at m[11 k ..], its degree at m[121 + k], root k at m[FP_ROOTS_AT + k] (a root is indexed by a loop counter too).
// Every member is divided by its largest coefficient, a positive factor
template <int S>
MPL_HD double horner(Strided<S> m, int at, int deg, double z) {
    double v = m[at + deg];
    for (int k = deg - 1; k >= 0; --k) v = v * z + m[at + k];
    return v;
}

template <int S>
MPL_HD int trimmed_degree(Strided<S> m, int at, int deg, double& big) {
    big = 0.0;
    for (int k = 0; k <= deg; ++k) big = fmax(big, fabs(m[at + k]));
    while (deg >= 0 && !(fabs(m[at + deg]) > FP_TRIM * big)) --deg;
    return deg;                              // -1: the zero polynomial (or one that is not a number)
}

template <int S>
MPL_HD int sturm_changes(Strided<S> m, int members, double z) {
    int changes = 0;
    double last = 0.0;
    for (int k = 0; k < members; ++k) {
        const double v = horner(m, 11 * k, (int)m[121 + k], z);
        if (v != 0.0) {
            if (last != 0.0 && (v < 0.0) != (last < 0.0)) ++changes;
            last = v;
        }
    }
    return changes;
}

template <int S>
MPL_HD int real_roots(Strided<S> m, const double (&p)[11]) {
#pragma unroll
    for (int k = 0; k < 11; ++k) m[k] = p[k];
    double big;
    int deg = trimmed_degree(m, 0, 10, big);
    if (deg < 1) return 0;
    for (int k = 0; k <= deg; ++k) m[k] = m[k] / big;
    m[121] = (double)deg;
    for (int k = 0; k < deg; ++k) m[11 + k] = (double)(k + 1) * m[k + 1];
    m[121 + 1] = (double)(deg - 1);
    int members = 2;
    // p_{k+1} = -rem(p_{k-1}, p_k), until a constant or nothing is left
    while ((int)m[121 + members - 1] > 0) {
        const int hi = 11 * (members - 2), lo = 11 * (members - 1), out = 11 * members;
        const int dh = (int)m[121 + members - 2], dl = (int)m[121 + members - 1];
        for (int k = 0; k <= dh; ++k) m[out + k] = m[hi + k];
        for (int i = dh; i >= dl; --i) {
            const double q = m[out + i] / m[lo + dl];
            for (int k = 0; k < dl; ++k) m[out + i - dl + k] -= q * m[lo + k];
            m[out + i] = 0.0;
        }
        double scale;
        const int dr = trimmed_degree(m, out, dl - 1, scale);
        if (dr < 0 || !(scale > FP_TRIM)) break;                 // the remainder vanishes: p has a repeated factor
        for (int k = 0; k <= dr; ++k) m[out + k] = -m[out + k] / scale;
        m[121 + members] = (double)dr;
        ++members;
    }
    // Cauchy's bound on the roots
    double bound = 0.0;
    for (int k = 0; k < deg; ++k) bound = fmax(bound, fabs(m[k] / m[deg]));
    bound += 1.0;
    const int at_low = sturm_changes(m, members, -bound);
    int n = at_low - sturm_changes(m, members, bound);
    n = n < 0 ? 0 : n > FP_MAX_ROOTS ? FP_MAX_ROOTS : n;
    for (int k = 0; k < n; ++k) {
        // root k from the left: the interval (lo, hi] shrinks until it holds that root alone
        double lo = -bound, hi = bound;
        int below = 0, within = n;           // roots in (-bound, lo] and in (lo, hi]
        for (int it = 0; it < FP_ISOLATE && within > 1; ++it) {
            const double mid = 0.5 * (lo + hi);
            const int left = at_low - sturm_changes(m, members, mid) - below;       // roots in (lo, mid]
            if (below + left > k) {
                hi = mid;
                within = left;
            } else {
                lo = mid;
                below += left;
                within -= left;
            }
        }
        double flo = horner(m, 0, deg, lo), fhi = horner(m, 0, deg, hi);
        double z = 0.5 * (lo + hi);
        if (fhi == 0.0) {
            z = hi;
        } else if ((flo < 0.0) != (fhi < 0.0) && flo != 0.0) {
            for (int it = 0; it < FP_BISECT; ++it) {
                z = 0.5 * (lo + hi);
                if (!(z > lo && z < hi)) break;                  // the two ends are neighbours
                const double fz = horner(m, 0, deg, z);
                if (fz == 0.0) break;
                if ((fz < 0.0) != (flo < 0.0)) hi = z;
                else lo = z;
            }
            for (int it = 0; it < FP_NEWTON; ++it) {
                const double fz = horner(m, 0, deg, z), dz = horner(m, 11, deg - 1, z);
                const double next = z - fz / dz;
                if (next >= lo && next <= hi) z = next;
            }
        }
        m[FP_ROOTS_AT + k] = z;
    }
    return n;
}

// ---- (x, y) at a root z: the null vector of B(z), the cross product of the two rows that make the longest one (the lowest pair
// among equals); false where its last entry is zero or the result is not finite
MPL_HD bool xy_at(const double (&Bz)[3][13], double z, double& x, double& y) {
    double v[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        v[r][0] = ((Bz[r][3] * z + Bz[r][2]) * z + Bz[r][1]) * z + Bz[r][0];
        v[r][1] = ((Bz[r][7] * z + Bz[r][6]) * z + Bz[r][5]) * z + Bz[r][4];
        v[r][2] = (((Bz[r][12] * z + Bz[r][11]) * z + Bz[r][10]) * z + Bz[r][9]) * z + Bz[r][8];
    }
    double c[3] = {0.0, 0.0, 0.0}, len = -1.0;
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
        const int i = pair == 2 ? 1 : 0, j = pair == 0 ? 1 : 2;
        const double c0 = v[i][1] * v[j][2] - v[i][2] * v[j][1], c1 = v[i][2] * v[j][0] - v[i][0] * v[j][2],
                     c2 = v[i][0] * v[j][1] - v[i][1] * v[j][0];
        const double l = c0 * c0 + c1 * c1 + c2 * c2;
        if (l > len) {
            len = l;
            c[0] = c0; c[1] = c1; c[2] = c2;
        }
    }
    x = c[0] / c[2];
    y = c[1] / c[2];
    return c[2] != 0.0 && fabs(x) <= 1.79769313486231570815e308 && fabs(y) <= 1.79769313486231570815e308;
}

MPL_HD double pick3(const double (&v)[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

// ---- the pose of an essential matrix (row-major): E = U diag(s) V^T by factor3 of hestenes.hpp, u3 = u1 x u2 and V proper;
// R in {U W V^T, U W^T V^T}, t = +-u3 in the order (R1, +), (R1, -), (R2, +), (R2, -); the first combination under which the five
// samples have positive depth in both cameras is kept.  pose: R row-major, then t.  false: none does, or E has no two singular values
MPL_HD bool pose_of(const double (&E)[9], const double (&ya)[FP_SAMPLE][2], const double (&yb)[FP_SAMPLE][2], double (&pose)[12]) {
    double M[3][3] = {{E[0], E[1], E[2]}, {E[3], E[4], E[5]}, {E[6], E[7], E[8]}};
    double W[3][3], sv[3];
    const int last = factor3(M, W, sv);
    const int i1 = (last + 1) % 3, i2 = (last + 2) % 3;          // (i1, i2, last) is an even permutation: V stays proper
    const double s1 = pick3(sv, i1), s2 = pick3(sv, i2);
    if (!(s1 > 0.0) || !(s2 > 0.0) || !(s1 <= 1.79769313486231570815e308) || !(s2 <= 1.79769313486231570815e308)) return false;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u1[r] = pick3(M[r], i1) / s1;
        u2[r] = pick3(M[r], i2) / s2;
        v1[r] = pick3(W[r], i1);
        v2[r] = pick3(W[r], i2);
        v3[r] = pick3(W[r], last);
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
    u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
    u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    bool found = false;
#pragma unroll
    for (int combo = 0; combo < 4; ++combo) {
        const double sr = combo < 2 ? 1.0 : -1.0, st = (combo & 1) ? -1.0 : 1.0;
        double R[9], t[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) R[3 * r + c] = sr * (u2[r] * v1[c] - u1[r] * v2[c]) + u3[r] * v3[c];
            t[r] = st * u3[r];
        }
        bool front = true;
#pragma unroll
        for (int i = 0; i < FP_SAMPLE; ++i) {
            // l_a R d_a - l_b d_b = -t by its normal equations
            const double p0 = R[0] * ya[i][0] + R[1] * ya[i][1] + R[2], p1 = R[3] * ya[i][0] + R[4] * ya[i][1] + R[5],
                         p2 = R[6] * ya[i][0] + R[7] * ya[i][1] + R[8];
            const double q0 = -yb[i][0], q1 = -yb[i][1], q2 = -1.0;
            const double pp = p0 * p0 + p1 * p1 + p2 * p2, pq = p0 * q0 + p1 * q1 + p2 * q2, qq = q0 * q0 + q1 * q1 + q2 * q2;
            const double bp = -(p0 * t[0] + p1 * t[1] + p2 * t[2]), bq = -(q0 * t[0] + q1 * t[1] + q2 * t[2]);
            const double det = pp * qq - pq * pq;
            const double la = (bp * qq - bq * pq) / det, lb = (pp * bq - pq * bp) / det;
            front = front && la > FP_DEPTH_MIN && lb > FP_DEPTH_MIN;
        }
        if (front && !found) {
            found = true;
#pragma unroll
            for (int k = 0; k < 9; ++k) pose[k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) pose[9 + k] = t[k];
        }
    }
    if (found) {
#pragma unroll
        for (int k = 0; k < 12; ++k) found = found && fabs(pose[k]) <= 1.79769313486231570815e308;
    }
    return found;
}

// ---- (x, y, z) of a candidate polished on the ten cubics themselves (m holds them again, as constraints() left them): FP_POLISH
// Gauss-Newton steps, (J^T J) delta = -J^T f by the adjugate of the 3 x 3.  B(z) loses its rank by two where two candidates have
// nearly the same z, and (x, y) read off it are then only a start; the cubics tell the two apart.  A step that is not finite is
// not taken
template <int S>
MPL_HD void polish(Strided<S> m, double& x, double& y, double& z) {
    for (int it = 0; it < FP_POLISH; ++it) {
        const double x2 = x * x, y2 = y * y, z2 = z * z;
        const double mono[20] = {x2 * x, y2 * y, x2 * y, x * y2, x2 * z, x2, y2 * z, y2, x * y * z, x * y,
                                 x, x * z, x * z2, y, y * z, y * z2, 1.0, z, z2, z2 * z};
        const double dx[20] = {3.0 * x2, 0.0, 2.0 * x * y, y2, 2.0 * x * z, 2.0 * x, 0.0, 0.0, y * z, y, 1.0, z, z2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double dy[20] = {0.0, 3.0 * y2, x2, 2.0 * x * y, 0.0, 0.0, 2.0 * y * z, 2.0 * y, x * z, x, 0.0, 0.0, 0.0, 1.0, z, z2, 0.0, 0.0, 0.0, 0.0};
        const double dz[20] = {0.0, 0.0, 0.0, 0.0, x2, 0.0, y2, 0.0, x * y, 0.0, 0.0, x, 2.0 * x * z, 0.0, y, 2.0 * y * z, 0.0, 1.0, 2.0 * z, 3.0 * z2};
        double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int r = 0; r < 10; ++r) {
            double f = 0.0, j0 = 0.0, j1 = 0.0, j2 = 0.0;
#pragma unroll
            for (int c = 0; c < 20; ++c) {
                const double v = m[r * 20 + c];
                f += v * mono[c];
                j0 += v * dx[c];
                j1 += v * dy[c];
                j2 += v * dz[c];
            }
            h00 += j0 * j0; h01 += j0 * j1; h02 += j0 * j2; h11 += j1 * j1; h12 += j1 * j2; h22 += j2 * j2;
            g0 += j0 * f; g1 += j1 * f; g2 += j2 * f;
        }
        const double a00 = h11 * h22 - h12 * h12, a01 = h02 * h12 - h01 * h22, a02 = h01 * h12 - h02 * h11;
        const double a11 = h00 * h22 - h02 * h02, a12 = h01 * h02 - h00 * h12, a22 = h00 * h11 - h01 * h01;
        const double det = h00 * a00 + h01 * a01 + h02 * a02;
        const double s0 = (a00 * g0 + a01 * g1 + a02 * g2) / det, s1 = (a01 * g0 + a11 * g1 + a12 * g2) / det,
                     s2 = (a02 * g0 + a12 * g1 + a22 * g2) / det;
        if (fabs(s0) <= 1.79769313486231570815e308 && fabs(s1) <= 1.79769313486231570815e308 && fabs(s2) <= 1.79769313486231570815e308) {
            x -= s0;
            y -= s1;
            z -= s2;
        }
    }
}

// ---- the solver up to the roots: basis, B(z) and the roots of det B(z), left at m[FP_ROOTS_AT ..] -> their number (0 where the
// elimination fails); m holds the ten cubics afterwards
template <int S>
MPL_HD int solve(Strided<S> m, const double (&ya)[FP_SAMPLE][2], const double (&yb)[FP_SAMPLE][2], double (&basis)[4][9],
                    double (&Bz)[3][13]) {
    null_space(m, ya, yb, basis);
    constraints(m, basis);
    if (!eliminate(m)) return 0;
    hidden_variable(m, Bz);
    double p[11];
    determinant(Bz, p);
    const int n = real_roots(m, p);
    // the cubics once more, for polish(): the elimination worked in place.  B(z) waits in the lane's storage meanwhile, so that
    // its 39 registers are free while the cubics are formed
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 13; ++k) m[FP_BZ_AT + 13 * r + k] = Bz[r][k];
    }
    // and the basis is made opaque: the compiler would otherwise keep the 200 coefficients of the first formation in registers
    // across the elimination and the root finder instead of forming them again, and spill
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int e = 0; e < 9; ++e) MPL_FP_OPAQUE(basis[k][e]);
    }
    constraints(m, basis);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 13; ++k) Bz[r][k] = m[FP_BZ_AT + 13 * r + k];
    }
    return n;
}

// the essential matrix of the candidate at root z, (x, y, z) polished -> false where (x, y) cannot be formed
template <int S>
MPL_HD bool essential_at(Strided<S> m, const double (&basis)[4][9], const double (&Bz)[3][13], double z, double (&E)[9]) {
    double x, y;
    const bool ok = xy_at(Bz, z, x, y);
    polish(m, x, y, z);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = x * basis[0][e] + y * basis[1][e] + z * basis[2][e] + basis[3][e];
    return ok;
}

}  // namespace fivept
}  // namespace mpl
