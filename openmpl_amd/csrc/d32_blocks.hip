// The D = 32 FPT block kernels of the joints x views token grid.
// The FPT blocks of the keypoint-token variant (FPT_blocks_view_keypoint_tokens: 17 V tokens of width 32, :261-266, :436-437)
// have the SPT block's Linear shapes, so they run from the same packed operand (spt_pack.hpp, written by mpl_spt_pack with the
// q columns unscaled) with the same arithmetic: two fp16 parts per operand, three partial products.  Everything except the
// attention is ROW-LOCAL at this width: a wave (512 threads = 8 waves per workgroup) takes a 16-row tile through a whole chain
// of GEMMs by itself -- weights in registers for all its tiles, the accumulator layout (lane = row i, 4 columns) turned into
// the next A fragment (lane = row i, 8 consecutive k) through a 16-row scratch tile of its own in LDS, no workgroup barrier
// anywhere:
//   d32_qkv_kernel:  qkv = LN1(x) . Wqkv^T + b                                         (-> token attention kernel)
//   d32_mlp_kernel:  x += att . Wproj^T + b;  x += fc2(gelu(fc1(LN2(x))))              (Block.forward :84-92, Mlp :31-37)
#include "spt_pack.hpp"

namespace mpl {

constexpr int SD = 32;          // token width
constexpr int XS = 36, HS = 68; // row strides (floats) of a wave's scratch tiles: x [16][36], hidden [16][68]

__global__ __launch_bounds__(512) void d32_qkv_kernel(const float* __restrict__ x, int M, const char* __restrict__ pack,
                                                       float* __restrict__ qkv) {
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int gw = blockIdx.x * 8 + (threadIdx.x >> 6), nw = gridDim.x * 8;
    const float* vec = reinterpret_cast<const float*>(pack + SPT_PACK_VEC);
    sf16x8 wq[6][2];
    float4 cq[6], sq[6];
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        spt_load_unit(pack, n, lane, wq[n]);
        cq[n] = ld4(vec + SPT_C_QKV + 16 * n + 4 * kq);
        sq[n] = ld4(vec + SPT_NCOL + SPT_C_QKV + 16 * n + 4 * kq);
    }
    const int n_tiles = (M + 15) / 16;
    // the rows of the NEXT tile of this wave are requested before the current one is multiplied (a wave walks ~4 tiles; one
    // memory round trip per tile in the open was most of the kernel's time)
    auto rows_of = [&](int tile, float4& a0, float4& a1) {
        const int r = tile * 16 + li;
        const float* xr = x + (size_t)(r < M ? r : M - 1) * SD + 8 * kq;
        a0 = ld4(xr);
        a1 = ld4(xr + 4);
    };
    float4 n0 = {0.f, 0.f, 0.f, 0.f}, n1 = n0;
    if (gw < n_tiles) rows_of(gw, n0, n1);
    for (int tile = gw; tile < n_tiles; tile += nw) {
        const int row = tile * 16 + li;
        const bool ok = row < M;
        const float4 c0 = n0, c1 = n1;
        if (tile + nw < n_tiles) rows_of(tile + nw, n0, n1);
        sf16x8 ah, al;
        spt_ln_split(c0, c1, ah, al);
        float* o = qkv + (size_t)row * (3 * SD) + 4 * kq;
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            const f32x4 c = mfma3(wq[n], ah, al, f32x4{0.f, 0.f, 0.f, 0.f});
            if (ok) st4(o + 16 * n, float4{fmaf(c[0], sq[n].x, cq[n].x), fmaf(c[1], sq[n].y, cq[n].y), fmaf(c[2], sq[n].z, cq[n].z),
                                           fmaf(c[3], sq[n].w, cq[n].w)});
        }
    }
}

__global__ __launch_bounds__(512) void d32_mlp_kernel(float* __restrict__ x, const float* __restrict__ att, int M,
                                                       const char* __restrict__ pack) {
    __shared__ __attribute__((aligned(16))) float scratch[8][16 * XS + 16 * HS];
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 8 + wave, nw = gridDim.x * 8;
    float* XT = scratch[wave];              // [16][36]: x after the attention half, in A-fragment order for norm2
    float* HT = XT + 16 * XS;               // [16][68]: the hidden layer (already times the static scale of the fc2 operand)
    const float* vec = reinterpret_cast<const float*>(pack + SPT_PACK_VEC);
    sf16x8 wp[2][2], w1[4][2], w2[2][2][2];
    float4 bp[2], sp[2], b1[4], s1[4], b2[2], s2[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        spt_load_unit(pack, 6 + n, lane, wp[n]);
        spt_load_unit(pack, 12 + 2 * n, lane, w2[n][0]);
        spt_load_unit(pack, 12 + 2 * n + 1, lane, w2[n][1]);
        bp[n] = ld4(vec + SPT_C_PROJ + 16 * n + 4 * kq);
        sp[n] = ld4(vec + SPT_NCOL + SPT_C_PROJ + 16 * n + 4 * kq);
        b2[n] = ld4(vec + SPT_C_FC2 + 16 * n + 4 * kq);
        s2[n] = ld4(vec + SPT_NCOL + SPT_C_FC2 + 16 * n + 4 * kq);
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        spt_load_unit(pack, 8 + n, lane, w1[n]);
        b1[n] = ld4(vec + SPT_C_FC1 + 16 * n + 4 * kq);
        s1[n] = ld4(vec + SPT_NCOL + SPT_C_FC1 + 16 * n + 4 * kq);
    }
    const float s_att = vec[2 * SPT_NCOL], hs = vec[2 * SPT_NCOL + 1];
    const int n_tiles = (M + 15) / 16;
    // operands of the NEXT tile of this wave (attention rows as A fragment, x in accumulator layout) are requested up front
    auto rows_of = [&](int tile, float4& a0, float4& a1, float4 (&xo)[2]) {
        const int r = tile * 16 + li;
        const size_t rcl = (size_t)(r < M ? r : M - 1);
        a0 = ld4(att + rcl * SD + 8 * kq);
        a1 = ld4(att + rcl * SD + 8 * kq + 4);
        xo[0] = ld4(x + rcl * SD + 4 * kq);
        xo[1] = ld4(x + rcl * SD + 16 + 4 * kq);
    };
    float4 na0 = {0.f, 0.f, 0.f, 0.f}, na1 = na0, nx[2] = {na0, na0};
    if (gw < n_tiles) rows_of(gw, na0, na1, nx);
    for (int tile = gw; tile < n_tiles; tile += nw) {
        const int row = tile * 16 + li;
        const bool ok = row < M;
        // ---- x += att . Wproj^T + b
        float4 xn[2];
        {
            const float4 a0 = na0, a1 = na1;
            const float4 xc[2] = {nx[0], nx[1]};
            if (tile + nw < n_tiles) rows_of(tile + nw, na0, na1, nx);
            const float y[8] = {a0.x * s_att, a0.y * s_att, a0.z * s_att, a0.w * s_att, a1.x * s_att, a1.y * s_att, a1.z * s_att, a1.w * s_att};
            sf16x8 ah, al;
            spt_split2(y, ah, al);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const f32x4 c = mfma3(wp[n], ah, al, f32x4{0.f, 0.f, 0.f, 0.f});
                const float4 xo = xc[n];
                xn[n] = float4{xo.x + fmaf(c[0], sp[n].x, bp[n].x), xo.y + fmaf(c[1], sp[n].y, bp[n].y), xo.z + fmaf(c[2], sp[n].z, bp[n].z),
                               xo.w + fmaf(c[3], sp[n].w, bp[n].w)};
                st4(XT + li * XS + 16 * n + 4 * kq, xn[n]);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's own LDS stores, read back in another lane order
        // ---- hidden = gelu(LN2(x) . W1^T + b)
        {
            sf16x8 ah, al;
            spt_ln_split(ld4(XT + li * XS + 8 * kq), ld4(XT + li * XS + 8 * kq + 4), ah, al);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const f32x4 c = mfma3(w1[n], ah, al, f32x4{0.f, 0.f, 0.f, 0.f});
                st4(HT + li * HS + 16 * n + 4 * kq,
                    float4{gelu_as_scaled(fmaf(c[0], s1[n].x, b1[n].x), hs), gelu_as_scaled(fmaf(c[1], s1[n].y, b1[n].y), hs),
                           gelu_as_scaled(fmaf(c[2], s1[n].z, b1[n].z), hs), gelu_as_scaled(fmaf(c[3], s1[n].w, b1[n].w), hs)});
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- x += hidden . W2^T + b   (K = 64: two k steps)
        {
            sf16x8 ah0, al0, ah1, al1;
            {
                const float4 h0 = ld4(HT + li * HS + 8 * kq), h1 = ld4(HT + li * HS + 8 * kq + 4);
                const float y[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
                spt_split2(y, ah0, al0);
            }
            {
                const float4 h0 = ld4(HT + li * HS + 32 + 8 * kq), h1 = ld4(HT + li * HS + 32 + 8 * kq + 4);
                const float y[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
                spt_split2(y, ah1, al1);
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                f32x4 c = mfma3(w2[n][0], ah0, al0, f32x4{0.f, 0.f, 0.f, 0.f});
                c = mfma3(w2[n][1], ah1, al1, c);
                if (ok) st4(x + (size_t)row * SD + 16 * n + 4 * kq,
                            float4{xn[n].x + fmaf(c[0], s2[n].x, b2[n].x), xn[n].y + fmaf(c[1], s2[n].y, b2[n].y),
                                   xn[n].z + fmaf(c[2], s2[n].z, b2[n].z), xn[n].w + fmaf(c[3], s2[n].w, b2[n].w)});
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the scratch tiles are rewritten by the next tile
    }
}

static int d32_grid(int M) {
    const int need = ((M + 15) / 16 + 7) / 8;
    return need < 512 ? (need > 0 ? need : 1) : 512;
}
int launch_d32_qkv(const float* x, int M, const unsigned short* pack, float* qkv, hipStream_t s) {
    if (!x || !pack || !qkv || M <= 0) return MPL_E_INVALID;
    ProfScope prof(MPL_K_GEMM, s);
    hipLaunchKernelGGL(d32_qkv_kernel, dim3(d32_grid(M)), dim3(512), 0, s, x, M, reinterpret_cast<const char*>(pack), qkv);
    return hip_check_launch();
}
int launch_d32_mlp(float* x, const float* att, int M, const unsigned short* pack, hipStream_t s) {
    if (!x || !pack || !att || M <= 0) return MPL_E_INVALID;
    ProfScope prof(MPL_K_GEMM, s);
    hipLaunchKernelGGL(d32_mlp_kernel, dim3(d32_grid(M)), dim3(512), 0, s, x, att, M, reinterpret_cast<const char*>(pack));
    return hip_check_launch();
}

}  // namespace mpl
