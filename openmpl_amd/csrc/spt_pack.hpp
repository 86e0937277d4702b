// The packed block of mpl_spt_pack and the arithmetic on it: the D = 32 Linear layers of a block (qkv 32 -> 96, proj 32 -> 32,
// fc1 32 -> 64, fc2 64 -> 32) as fp32 GEMMs on the fp16 matrix cores from operands split in TWO fp16 parts, x = hi + lo, THREE
// partial products (lo.hi, hi.lo, hi.hi), fp32 accumulation, exact power-of-two scales -- the arithmetic of h2_gemm.hip.
// Written by spt_pack_kernel (spt_packed.hip); read by spt3_kernel<SS> (spt_packed.hip) and by the D = 32 FPT block kernels
// (d32_blocks.hip).
//
// Layout: fragments [16 units][hi | lo][64 lanes][8 fp16], a unit = one 16-column tile x one 32-deep k step (2 KiB): 6 qkv,
// 2 proj, 4 fc1, 4 fc2 = (n tile, k step); lane (li, kq) of a unit holds k = 8 kq .. 8 kq + 7 of weight row 16 n + li, times
// the column scale sw_n.  Then, at byte SPT_PACK_VEC, the fp32 epilogue vectors c[224] | sc[224] | {s_att, s_hid / 2, 0 ..}:
// y_n = acc_n sc_n + c_n; columns qkv 0..95, proj 96.., fc1 128.., fc2 192.. (how c, sc and the scales are formed: spt_pack_kernel).
#pragma once
#include "common.hpp"

namespace mpl {

constexpr int SPT_PACK_QKV = 0, SPT_PACK_PROJ = 12 * 1024, SPT_PACK_FC1 = 16 * 1024, SPT_PACK_FC2 = 24 * 1024;
constexpr int SPT_PACK_VEC = 32 * 1024;
constexpr int SPT_PACK_BYTES = 48 * 1024;
constexpr int SPT_C_QKV = 0, SPT_C_PROJ = 96, SPT_C_FC1 = 128, SPT_C_FC2 = 192, SPT_NCOL = 224;
constexpr int SPT3_NPAR = 456;                      // floats of epilogue vectors per block: c[224] | sc[224] | scalars[8]
constexpr float SPT_SA = 1024.0f;                   // scale of a normalised LayerNorm input (|z| <= sqrt(32))
constexpr float SPT_QS = 0.5f * 1.4426950408889634f;   // hd^-0.5 log2 e, folded into the q columns (scores in the exp2 domain)

typedef _Float16 sf16x8 __attribute__((ext_vector_type(8)));

// 8 fp32 -> hi / lo packed fp16 (RNE; the residual is exact in fp32; subnormal results are kept): h2_gemm.hip
__device__ __forceinline__ void spt_split2(const float (&x)[8], sf16x8& hi, sf16x8& lo) { ::mpl::split2_f16(x, hi, lo); }     // common.hpp

// acc(16 x 16, transposed) += the three significant part products of A (hi, lo) and W (hi, lo): lo.hi, hi.lo, hi.hi
__device__ __forceinline__ f32x4 mfma3(const sf16x8 (&w)[2], const sf16x8& ah, const sf16x8& al, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[0], al, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[1], ah, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[0], ah, c, 0, 0, 0);
    return c;
}

// Normalised, split A fragment of a 32-wide row held by the 4 lanes {i, i + 16, i + 32, i + 48}, 8 consecutive k each (a0 | a1):
// z = (x - mean) rstd 2^10 (gamma / beta live in the packed weights / c); mean and variance are two lane swaps each
__device__ __forceinline__ void spt_ln_split(const float4& a0, const float4& a1, sf16x8& ah, sf16x8& al) {
    float4 x0 = a0, x1 = a1;
    float sm = ((x0.x + x0.y) + (x0.z + x0.w)) + ((x1.x + x1.y) + (x1.z + x1.w));
    sm = xor32_add(xor16_add(sm));
    const float mean = sm * (1.0f / 32.0f);
    x0.x -= mean; x0.y -= mean; x0.z -= mean; x0.w -= mean;
    x1.x -= mean; x1.y -= mean; x1.z -= mean; x1.w -= mean;
    float ss = ((x0.x * x0.x + x0.y * x0.y) + (x0.z * x0.z + x0.w * x0.w)) + ((x1.x * x1.x + x1.y * x1.y) + (x1.z * x1.z + x1.w * x1.w));
    ss = xor32_add(xor16_add(ss));
    const float rs = __builtin_amdgcn_rsqf(ss * (1.0f / 32.0f) + 1e-6f) * SPT_SA;   // v_rsq_f32 (1 ulp)
    const float y[8] = {x0.x * rs, x0.y * rs, x0.z * rs, x0.w * rs, x1.x * rs, x1.y * rs, x1.z * rs, x1.w * rs};
    spt_split2(y, ah, al);
}
// this lane's hi | lo fragments of unit `unit` counted from `base` (a packed block or a section of one, in global memory or LDS)
__device__ __forceinline__ void spt_load_unit(const char* base, int unit, int lane, sf16x8 (&w)[2]) {
    const sf16x8* g = reinterpret_cast<const sf16x8*>(base) + (size_t)unit * 2 * 64 + lane;
    w[0] = g[0];
    w[1] = g[64];
}

}  // namespace mpl
