// Shape-general bf16 GEMMs of the FPT block stack ("bf16" matmul precision for every view-token model whose width the tuned
// engine of b1_gemm.hip does not take):
//     Y[M][N] = epi( A[M][K] . W16[N][K]^T ... ),   operands rounded to bf16, products exact, fp32 accumulation
// for run-time M, N, K.  ONE plain launch per GEMM: no persistent kernel, no hand-off between workgroups, no waits.
//
// Reference ops (MPL/lib/models/multiview_mpl.py): Block.norm1 + Attention.qkv :55, Attention.proj :65 + residual :90,
// Block.norm2 + Mlp.fc1 + GELU :32-33, Mlp.fc2 :35 + residual :91.  Rounding points: oracle/mpl_oracle.py block_bf16.
//
// Tile: 64 rows x 64 columns per workgroup of 4 waves; wave w owns rows 16 w .. 16 w + 15 and all four 16-column tiles, one
// v_mfma_f32_16x16x32_bf16 per (k-tile of 32, column tile).  The k-tiles are walked 0 .. KT - 1 whatever M is, and a row's
// accumulators see only that row of A: a row's result depends on (N, K) alone, not on M or on where the row sits in the batch.
//   W: the packed operand of mpl_pack_bf16_any -- [ceil(N/64)][KT = ceil(K/32)][4 column tiles][64 lanes][8 bf16], lane l of a
//      fragment = column 16 t + (l & 15), k = 32 kt + 8 (l >> 4) + j, ZERO beyond N and K (so the k loop has no tail code),
//      followed by fp32 c[N] = bias + W.beta and s[N] = sum_k bf16(gamma_k W_nk).  One k-tile of a column block is 4 KiB: every
//      thread brings 16 bytes to LDS (two buffers, one barrier per k-tile), every wave reads all four fragments back.
//   A: each wave reads the fragment of its own 16 rows straight from global memory (no other wave needs it), one k-tile ahead:
//      LayerNorm GEMMs (qkv, fc1) the raw fp32 residual rows, rounded to bf16 (nearest even) in registers;
//      plain GEMMs (proj, fc2) bf16 rows of leading dimension b1a_ld(K) (a multiple of 32: every 16-byte read stays inside its
//      row).  Elements at k >= K and rows >= M are masked to zero / clamped on the way in, never trusted to be zero.
//   The LayerNorm is folded: rstd (x16 . (gamma o W)16^T - mean s) + c, mean / rstd (eps 1e-6) combined in the epilogue from the
//      fp32 slice partials of launch_row_stats (gemm_common.hpp ln_combine).
#include "gemm_common.hpp"

namespace mpl {

namespace {

typedef __bf16 a_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned a_u32x4 __attribute__((ext_vector_type(4)));

constexpr int TA_M = 64, TA_N = 64, TA_K = 32;
constexpr int TA_WB = TA_N * TA_K * 2;          // bytes of one k-tile of a column block: 4 fragments of 1 KiB

inline int ta_nb(int N) { return (N + TA_N - 1) / TA_N; }
inline int ta_kt(int K) { return (K + TA_K - 1) / TA_K; }

__device__ __forceinline__ unsigned short bf16_bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }

// ---------------------------------------------------------------------------------------------- weight operand
// c_n = b_n + sum_k beta_k W_nk and s_n = sum_k of the ROUNDED gamma_k W_nk (fp64 sums), one wave per output column
__global__ __launch_bounds__(256) void b1a_fold_kernel(const float* __restrict__ W, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ bias, int N, int K,
                                                        float* __restrict__ tr) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    double sv = 0.0, c = 0.0;
    if (gamma) {
        for (int k = lane; k < K; k += 64) {
            const float w = W[(size_t)n * K + k];
            sv += (double)(float)(__bf16)(w * gamma[k]);
            c += (double)w * (double)beta[k];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sv += __shfl_xor(sv, o, 64);
            c += __shfl_xor(c, o, 64);
        }
    }
    if (lane == 0) {
        tr[n] = (float)(c + (double)bias[n]);
        tr[N + n] = (float)sv;
    }
}

__global__ __launch_bounds__(256) void b1a_pack_w_kernel(const float* __restrict__ W, const float* __restrict__ gamma, int N, int K,
                                                          a_bf16x8* __restrict__ dst, size_t total) {
    const int KT = (K + TA_K - 1) / TA_K;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int lane = (int)(idx & 63), t = (int)((idx >> 6) & 3);
        const int kt = (int)((idx >> 8) % KT), nb = (int)((idx >> 8) / KT);
        const int n = nb * TA_N + t * 16 + (lane & 15), k0 = kt * TA_K + 8 * (lane >> 4);
        a_bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = 0.f;
            if (n < N && k0 + j < K) {
                const float w = W[(size_t)n * K + k0 + j];
                x = gamma ? w * gamma[k0 + j] : w;          // LayerNorm gain folded into the weight (one fp32 rounding)
            }
            v[j] = (__bf16)x;
        }
        dst[idx] = v;       // idx = ((nb KT + kt) 4 + t) 64 + lane
    }
}

// fp32 rows -> bf16 rows of leading dimension ld (zeros behind column K): the A operand of a plain GEMM (mpl_ln_linear_bf16_any)
__global__ __launch_bounds__(256) void b1a_rows_kernel(const float* __restrict__ X, int M, int K, int ld, unsigned short* __restrict__ dst) {
    const size_t total = (size_t)M * ld;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t r = idx / ld;
        const int c = (int)(idx - r * ld);
        dst[idx] = c < K ? bf16_bits(X[r * K + c]) : (unsigned short)0;
    }
}

// ---------------------------------------------------------------------------------------------- the GEMM
struct B1aArgs {
    const float* X;             // LN: fp32 rows [M][ldx]
    const unsigned short* A16;  // plain: bf16 rows [M][lda], lda % 32 == 0
    const a_u32x4* W;           // packed operand
    const float *c, *s;         // trailer vectors
    const float* stats;         // LN: slice partials of launch_row_stats
    const float* R;             // residual rows [M][ldc] (may alias C)
    void* C;                    // fp32 [M][ldc], or bf16 [M][ldc] behind the GELU
    int M, N, K, ldx, lda, ldc, KT;
    int sl;                     // LN: slice length of the partials (ln_slice_len(K))
    float eps;
};

// the A fragment of k-tile kt: 8 consecutive k of row `row` (already clamped to < M), masked to zero at k >= K
template <bool LN, bool VEC>
__device__ __forceinline__ void b1a_load_a(const B1aArgs& a, int row, int k0, float (&xf)[8], a_u32x4& xb) {
    if constexpr (LN) {
        const float* p = a.X + (size_t)row * a.ldx + k0;
        if constexpr (VEC) {        // K % 4 == 0 and ldx % 4 == 0: a float4 is inside the row or wholly behind it
            const float4 z = {0.f, 0.f, 0.f, 0.f};
            const float4 u = k0 + 4 <= a.K ? ld4(p) : z, v = k0 + 8 <= a.K ? ld4(p + 4) : z;
            xf[0] = u.x; xf[1] = u.y; xf[2] = u.z; xf[3] = u.w; xf[4] = v.x; xf[5] = v.y; xf[6] = v.z; xf[7] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) xf[j] = k0 + j < a.K ? p[j] : 0.f;
        }
    } else {
        xb = *reinterpret_cast<const a_u32x4*>(a.A16 + (size_t)row * a.lda + k0);      // k0 + 7 < lda: inside the row
        const int rem = a.K - k0;
#pragma unroll
        for (int p = 0; p < 4; ++p) xb[p] &= (2 * p < rem ? 0xffffu : 0u) | (2 * p + 1 < rem ? 0xffff0000u : 0u);
    }
}

template <bool LN, bool VEC, int EPI>
__global__ __launch_bounds__(256) void b1a_gemm_kernel(const B1aArgs a) {
    __shared__ a_u32x4 wsm[2][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int row0 = blockIdx.x * TA_M + wave * 16, nb = blockIdx.y;
    const int arow = row0 + li < a.M ? row0 + li : a.M - 1;
    const a_u32x4* wp = a.W + (size_t)nb * a.KT * 256 + tid;

    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    float xf[8];
    a_u32x4 xb = {0u, 0u, 0u, 0u};
    a_u32x4 wreg = wp[0];
    b1a_load_a<LN, VEC>(a, arow, 8 * kq, xf, xb);
    for (int kt = 0; kt < a.KT; ++kt) {
        wsm[kt & 1][tid] = wreg;
        a_bf16x8 af;
        if constexpr (LN) {
#pragma unroll
            for (int j = 0; j < 8; ++j) af[j] = (__bf16)xf[j];
        } else {
            af = __builtin_bit_cast(a_bf16x8, xb);
        }
        const int kn = kt + 1 < a.KT ? kt + 1 : kt;        // the last round re-reads its own tile: no branch, nothing out of bounds
        wreg = wp[(size_t)kn * 256];
        b1a_load_a<LN, VEC>(a, arow, kn * TA_K + 8 * kq, xf, xb);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const a_bf16x8 bf = __builtin_bit_cast(a_bf16x8, wsm[kt & 1][t * 64 + lane]);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[t], 0, 0, 0);
        }
    }

    // epilogue: acc[t][r] = D[row0 + 4 kq + r][nb 64 + 16 t + li]
    float mu[4], rs[4];
    if constexpr (LN) {
        const int sl = a.sl, ns = a.K / sl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = row0 + 4 * kq + r;
            mu[r] = 0.f;
            rs[r] = 0.f;
            if (m < a.M) ln_combine(a.stats + (size_t)m * ns * 2, ns, sl, a.K, a.eps, mu[r], rs[r]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = nb * TA_N + 16 * t + li;
        if (col >= a.N) continue;
        const float cn = a.c[col], sn = LN ? a.s[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = row0 + 4 * kq + r;
            if (m >= a.M) continue;
            float y = acc[t][r];
            if constexpr (LN) y = rs[r] * (y - mu[r] * sn) + cn;
            else y += cn;
            const size_t o = (size_t)m * a.ldc + col;
            if constexpr (EPI == MPL_EPI_BIAS_GELU) reinterpret_cast<unsigned short*>(a.C)[o] = bf16_bits(gelu_erf(y));
            else if constexpr (EPI == MPL_EPI_BIAS_RESIDUAL) reinterpret_cast<float*>(a.C)[o] = a.R[o] + y;
            else reinterpret_cast<float*>(a.C)[o] = y;
        }
    }
}

template <bool LN, bool VEC, int EPI>
int b1a_launch(const B1aArgs& a, hipStream_t s) {
    ProfScope prof(MPL_K_GEMM, s);
    hipLaunchKernelGGL((b1a_gemm_kernel<LN, VEC, EPI>), dim3((a.M + TA_M - 1) / TA_M, ta_nb(a.N)), dim3(256), 0, s, a);
    return hip_check_launch();
}

}  // namespace

// ---------------------------------------------------------------------------------------------- host side
int b1a_ld(int K) { return (K + 31) / 32 * 32; }

size_t b1a_operand_bytes(int N, int K) {
    if (N < 1 || K < 1 || N > 16384 || K > 8192) return 0;
    return ((size_t)ta_nb(N) * ta_kt(K) * TA_WB + (size_t)2 * N * sizeof(float) + 15) / 16 * 16;
}

int launch_pack_b1a(const float* W, int N, int K, const float* ln_w, const float* ln_b, const float* bias, unsigned short* dst,
                    hipStream_t s) {
    if (!W || !dst || !bias || b1a_operand_bytes(N, K) == 0 || ((ln_w != nullptr) != (ln_b != nullptr))) return MPL_E_INVALID;
    if (reinterpret_cast<uintptr_t>(dst) & 15) return MPL_E_INVALID;       // the operand is written and read as 16-byte fragments
    const size_t total = (size_t)ta_nb(N) * ta_kt(K) * 256;
    float* tr = reinterpret_cast<float*>(reinterpret_cast<char*>(dst) + total * 16);
    ProfScope prof(MPL_K_PACK, s);
    hipLaunchKernelGGL(b1a_fold_kernel, dim3((N + 3) / 4), dim3(256), 0, s, W, ln_w, ln_b, bias, N, K, tr);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(b1a_pack_w_kernel, dim3(grid), dim3(256), 0, s, W, ln_w, N, K, reinterpret_cast<a_bf16x8*>(dst), total);
    return hip_check_launch();
}

int launch_b1a_rows(const float* X, int M, int K, unsigned short* dst, hipStream_t s) {
    if (!X || !dst || M <= 0 || K <= 0) return MPL_E_INVALID;
    const size_t total = (size_t)M * b1a_ld(K);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    ProfScope prof(MPL_K_PACK, s);
    hipLaunchKernelGGL(b1a_rows_kernel, dim3(grid), dim3(256), 0, s, X, M, K, b1a_ld(K), dst);
    return hip_check_launch();
}

int launch_b1a_gemm(const float* X, int ldx, const unsigned short* A16, int lda, const unsigned short* W16, const float* stats, float eps,
                    const float* R, void* C, int ldc, int M, int N, int K, int epi, hipStream_t s) {
    if (M <= 0 || !W16 || !C || b1a_operand_bytes(N, K) == 0 || ldc < N || (reinterpret_cast<uintptr_t>(W16) & 15)) return MPL_E_INVALID;
    if ((long long)M > (1ll << 30)) return MPL_E_UNSUPPORTED;      // 32-bit rows; the row tiles ride on grid.x (2^31 - 1)
    const bool ln = X != nullptr;
    if (ln ? (!stats || ldx < K || A16) : (!A16 || lda < b1a_ld(K) || (lda & 7) || (reinterpret_cast<uintptr_t>(A16) & 15))) return MPL_E_INVALID;
    const char* w = reinterpret_cast<const char*>(W16);
    const float* vec = reinterpret_cast<const float*>(w + (size_t)ta_nb(N) * ta_kt(K) * TA_WB);
    const B1aArgs a{X, A16, reinterpret_cast<const a_u32x4*>(w), vec, vec + N, stats, R, C, M, N, K, ldx, lda, ldc, ta_kt(K), ln_slice_len(K), eps};
    if (ln) {
        const bool vec4 = (K & 3) == 0 && (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
        if (epi == MPL_EPI_BIAS) return vec4 ? b1a_launch<true, true, MPL_EPI_BIAS>(a, s) : b1a_launch<true, false, MPL_EPI_BIAS>(a, s);
        if (epi == MPL_EPI_BIAS_GELU)
            return vec4 ? b1a_launch<true, true, MPL_EPI_BIAS_GELU>(a, s) : b1a_launch<true, false, MPL_EPI_BIAS_GELU>(a, s);
        return MPL_E_UNSUPPORTED;
    }
    if (epi == MPL_EPI_BIAS_RESIDUAL && R) return b1a_launch<false, true, MPL_EPI_BIAS_RESIDUAL>(a, s);
    return MPL_E_UNSUPPORTED;
}

}  // namespace mpl
