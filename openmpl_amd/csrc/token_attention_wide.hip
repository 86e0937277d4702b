// Long token attention for wide heads: the joints x views token grid (FPT_blocks_view_keypoint_tokens) at head dims 16 .. 128.
//
// Reference: Attention.forward, MPL/lib/models/multiview_mpl.py:55-64 (the tensor contract of token_attention.hip).
// Envelope: hd % 16 == 0, 16 <= hd <= 128, 33 <= n_tok <= 2048, any n_seq / heads.  fp32 arithmetic throughout: both matrix
// products run on v_mfma_f32_16x16x4_f32 (exact fp32, bitwise an fmaf chain), the softmax on the VALU over the accumulator tile.
//
// K and V of a head do not fit in LDS here (2048 tokens x hd 64 x 2 x 4 B = 1 MiB), so they stream through it in tiles of
// WA_KT = 64 keys and the softmax is the online form: running maximum m, running sum l and an output accumulator per query row,
// the accumulator rescaled by exp2(m_old - m_new) whenever a tile raises the maximum.
//
// Work split: a workgroup owns one (sequence, head, tile of 16 * waves query rows); every wave owns 16 query rows and walks
// all key tiles; the workgroup's waves share the K / V tile in LDS.
//
// Both products are formed TRANSPOSED, so that a lane owns ONE query row from the scores to the store:
//   S^T (16 keys x 16 queries) = K Q^T     A = K rows from LDS (one 16-byte read feeds four MFMAs), B = Q from registers;
//                                          lane (q = l & 15, g = l >> 4) then holds S[q][key 16 c + 4 g + r] in register r of tile c
//   O^T (16 channels x 16 queries) += V^T P^T   over keys in steps of 4: step r of key tile c contracts the keys 16 c + 4 g' + r
//                                          (g' = 0..3), whose B operand P^T[key][q] is exactly register r of the lane's score tile --
//                                          the accumulator tile of the first product is the operand of the second with no lane
//                                          movement and no trip through LDS; A = V[key 16 c + 4 g + r][channel 16 n + (l & 15)].
//   Lane (q, g) ends up with O[q][16 n + 4 g + 0..3]: four consecutive channels, one 16-byte store.
// The k order of S^T is permuted inside each 16 channels (mfma16_k16: lane (., g) supplies channels 16 t + 4 g + 0..3, step
// u contracts {16 t + 4 g' + u}); a sum of products in another order, every product once.
// Row maximum: 16 scores in the lane, then across the four lanes g of a query (permlane16 / permlane32 swaps).  The row sum stays
// a per-lane partial (rescaled with the accumulator) and the four partials are added once at the end.
//
// LDS map (floats): K tile [64][hd + 4] | V tile [64][hd + 4]; 512 (hd + 4) bytes: 10 KiB at hd 16, 66 KiB at hd 128 (opt-in).
// The row pad of 4 floats makes both access patterns conflict free: the K read (lane (j, g): 16 bytes at row j, float 16 t + 4 g)
// puts the 16 rows of a quarter wave on 16 distinct bank quads ((hd + 4) j mod 64 is a permutation of the multiples of 4 because
// hd % 16 == 0), the V read (lane (c, g): float c of row 4 g + r) puts the four rows on banks 16 g + 0..15.
// Keys past n_tok in the last tile: K / V rows zero-filled in LDS (0 * garbage could be NaN), scores replaced by -inf, so their
// weight is exp2(-inf) = 0 exactly.  The first tile always holds a real key, so m is finite from the first tile on.
// Query rows past n_tok in the last query tile: read clamped, never stored; a wave without any real row skips the arithmetic
// (it still loads and meets the barriers).
//
// gfx950 resource use (hipcc -O3, no scratch in any instantiation): see the table next to the launcher.
#include "common.hpp"

namespace mpl {

constexpr int WA_KT = 64;       // keys per LDS tile = four 16-key score tiles per wave (four independent MFMA chains)
constexpr int WA_PAD = 4;       // floats of row padding in LDS
constexpr int WA_MAX_WAVES = 4;

// max(v[l], v[l ^ 16]) and max(v[l], v[l ^ 32]) in every lane (the swaps of xor16_add / xor32_add in common.hpp)
__device__ __forceinline__ float wa_xor16_max(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}
__device__ __forceinline__ float wa_xor32_max(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

template <int HD>
__global__ __launch_bounds__(64 * WA_MAX_WAVES) void token_attention_wide_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                                  int n_tok, int D, int H, int q_tiles, float qs) {
    static_assert(HD % 16 == 0 && HD >= 16 && HD <= 128, "head dim: a multiple of 16 up to 128");
    constexpr int NT = HD / 16;                 // 16-channel tiles of a head
    constexpr int LD = HD + WA_PAD;             // LDS row stride (floats)
    constexpr int C4 = HD / 4;                  // float4 per K / V row
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ks = sm;
    float* Vs = sm + WA_KT * LD;

    const int nthr = blockDim.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lq = lane & 15, g = lane >> 4;
    const int qt = blockIdx.x % q_tiles, sh = blockIdx.x / q_tiles;
    const int h = sh % H, sq = sh / H;
    const size_t ld = (size_t)3 * D;
    const float* base = qkv + (size_t)sq * n_tok * ld + (size_t)h * HD;

    const int qw0 = qt * (nthr >> 2) + 16 * wave;       // first query row of this wave (16 rows per wave)
    const bool active = qw0 < n_tok;                    // wave-uniform
    const int qi = qw0 + lq;
    const int qc = qi < n_tok ? qi : n_tok - 1;

    f32x4 q[NT];                                        // B operand of S^T: channels 16 t + 4 g + 0..3 of query row qc
#pragma unroll
    for (int t = 0; t < NT; ++t) q[t] = *reinterpret_cast<const f32x4*>(base + (size_t)qc * ld + 16 * t + 4 * g);
    f32x4 o[NT];                                        // O^T tiles: channels 16 n + 4 g + r of query row qi
#pragma unroll
    for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                       // running maximum (exp2 domain) and this lane's part of the running sum

    for (int j0 = 0; j0 < n_tok; j0 += WA_KT) {
        __syncthreads();                                // every wave is done with the previous tile
        for (int i = tid; i < WA_KT * C4; i += nthr) {
            const int r = i / C4, c = i - r * C4;
            float4 k = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + r < n_tok) {
                const float* row = base + (size_t)(j0 + r) * ld + 4 * c;
                k = ld4(row + D);
                v = ld4(row + 2 * D);
            }
            st4(Ks + r * LD + 4 * c, k);
            st4(Vs + r * LD + 4 * c, v);
        }
        __syncthreads();
        if (!active) continue;

        // ---- S^T = K Q^T: four 16-key tiles, HD / 4 chained steps each
        f32x4 s[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            f32x4 kf[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) kf[c] = *reinterpret_cast<const f32x4*>(Ks + (16 * c + lq) * LD + 16 * t + 4 * g);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = mfma16(kf[c][u], q[t][u], s[c]);
        }
        // ---- online softmax of query row qi over the lane's 16 keys 16 c + 4 g + r (exp2 domain: qs = hd^-0.5 log2 e)
        const bool ragged = j0 + WA_KT > n_tok;         // uniform: the last tile, with keys past the end
        float mc = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ragged && j0 + 16 * c + 4 * g + r >= n_tok) s[c][r] = -INFINITY;
                mc = fmaxf(mc, s[c][r]);
            }
        mc = wa_xor32_max(wa_xor16_max(mc)) * qs;       // qs > 0: the maximum of the scaled scores
        const float mn = fmaxf(m, mc);
        const float f = __builtin_amdgcn_exp2f(m - mn); // 1 when the tile does not raise the maximum, 0 on the first tile
        m = mn;
        l *= f;
#pragma unroll
        for (int n = 0; n < NT; ++n) o[n] *= f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[c][r], qs, -mn));
                s[c][r] = p;
                l += p;
            }
        // ---- O^T += V^T P^T: step (c, r) contracts the keys 16 c + 4 g' + r
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vrow = Vs + (16 * c + 4 * g + r) * LD + lq;
#pragma unroll
                for (int n = 0; n < NT; ++n) o[n] = mfma16(vrow[16 * n], s[c][r], o[n]);
            }
    }
    if (!active) return;
    l = xor32_add(xor16_add(l));
    if (qi >= n_tok) return;
    const float inv = 1.0f / l;
    float* orow = out + ((size_t)sq * n_tok + qi) * D + (size_t)h * HD + 4 * g;
#pragma unroll
    for (int n = 0; n < NT; ++n) st4(orow + 16 * n, float4{o[n][0] * inv, o[n][1] * inv, o[n][2] * inv, o[n][3] * inv});
}

bool token_attention_wide_ok(int n_tok, int hd) { return n_tok > 32 && n_tok <= 2048 && hd >= 16 && hd <= 128 && hd % 16 == 0; }

// gfx950 resources per instantiation (hipcc -O3 -save-temps: no scratch, no spill anywhere; arch + accumulation registers):
//   hd     16    32    48    64    80    96   112   128
//   VGPR   60    64    68    80    92   120   128   152     (+ 16 .. 44 AGPR)
//   LDS    10    18    26    34    42    50    58    66 KiB (hd 128 alone needs the opt-in above 64 KiB)
// UNMEASURED: the time per launch, and whether the matrix-pipe form beats a VALU form or the head-dim-4 kernel at equal FLOPs (n_seq 256,
// n_tok 527, D 32), have not been measured on a GPU.  tools/kptok_wide_prof.py measures both.
template <int HD>
static int launch_wide(const float* qkv, int n_seq, int n_tok, int dim, int heads, float* out, hipStream_t s) {
    // 16 query rows per wave, up to four waves per workgroup (they share the K / V tile)
    int waves = (n_tok + 15) / 16;
    waves = waves > WA_MAX_WAVES ? WA_MAX_WAVES : waves;
    const int q_tiles = (n_tok + 16 * waves - 1) / (16 * waves);
    const long long blocks = (long long)n_seq * heads * q_tiles;
    if (blocks * 64 * waves > 0xffffffffll) return MPL_E_UNSUPPORTED;      // HIP launches at most 2^32 - 1 threads per grid dimension
    constexpr int lds = 2 * WA_KT * (HD + WA_PAD) * (int)sizeof(float);
    if constexpr (lds > 64 * 1024) {
        if (int rc = kernel_lds_once<token_attention_wide_kernel<HD>>(lds)) return rc;
    }
    const float qs = 1.4426950408889634f / sqrtf((float)HD);
    ProfScope prof(MPL_K_ATTENTION, s);
    hipLaunchKernelGGL(token_attention_wide_kernel<HD>, dim3((unsigned)blocks), dim3(64 * waves), lds, s, qkv, out, n_tok, dim, heads,
                       q_tiles, qs);
    return hip_check_launch();
}

int launch_token_attention_wide(const float* qkv, int n_seq, int n_tok, int dim, int heads, float* out, hipStream_t s) {
    if (n_seq <= 0 || n_tok <= 0 || heads <= 0 || dim % heads) return MPL_E_INVALID;
    const int hd = dim / heads;
    if (!token_attention_wide_ok(n_tok, hd)) return MPL_E_UNSUPPORTED;
    switch (hd) {
        case 16: return launch_wide<16>(qkv, n_seq, n_tok, dim, heads, out, s);
        case 32: return launch_wide<32>(qkv, n_seq, n_tok, dim, heads, out, s);
        case 48: return launch_wide<48>(qkv, n_seq, n_tok, dim, heads, out, s);
        case 64: return launch_wide<64>(qkv, n_seq, n_tok, dim, heads, out, s);
        case 80: return launch_wide<80>(qkv, n_seq, n_tok, dim, heads, out, s);
        case 96: return launch_wide<96>(qkv, n_seq, n_tok, dim, heads, out, s);
        case 112: return launch_wide<112>(qkv, n_seq, n_tok, dim, heads, out, s);
        default: return launch_wide<128>(qkv, n_seq, n_tok, dim, heads, out, s);
    }
}

}  // namespace mpl
