// The SPT stage on the fp16 matrix cores -- what precision "fp32" runs (spt.hip: spt_form -> MPL_SPT_PACKED): spt_pack_kernel
// writes the packed block of a Block's four Linear layers once per binding (format and arithmetic: spt_pack.hpp -- two fp16
// parts per operand, three partial products, fp32 accumulation), spt3_kernel<SS> runs the whole stage from it.
//
// spt3_kernel<SS>, 512 threads = 8 waves, SS = 16, 8, 4, 2 or 1 sequences per workgroup:
//   * token-major rows (row = joint * SS + sequence) and the W fragment as FIRST MFMA operand: lane (s, kq) of an
//     accumulator tile holds 4 consecutive columns of one (joint, sequence) -- for the qkv tiles exactly the 4-dim vector
//     of ONE head (h = 4 hg + kq).  Wave (hg, part) computes q, k, v of head group hg for the row tiles m = part (mod 4):
//     q stays in registers, k / v go to LDS per (joint, head, sequence);
//   * attention: the lane keeps its (sequence, head) and its <= 5 query joints; every K / V row is read once
//     (contiguous wave reads) for all of them -- 34 ds_read_b128 per lane and block application;
//   * proj / fc1 / fc2: A fragments are read from LDS (attention output, normalised X, GELU output), split in registers
//     into two fp16 parts (~20 VALU ops per fragment) and multiplied with the packed weight fragments (LayerNorm gain / offset
//     and the biases folded in, staged in LDS one phase ahead): 816 fp16 MFMAs of 16 cycles per block application at SS = 16.
// LDS (floats): X[272][36] | K[17][8][SS][4] in 8704 | V[17][8][SS][4] in 8704 | ATT[272][36]; the MLP hidden HID[272][68]
// aliases K | V | ATT from 12 KiB into K; behind them 8 KiB of staged weights and 2 x 456 parameters (the map: SPT3_* below).
#include "spt_pack.hpp"
#include "spt_stage.hpp"

namespace mpl {

constexpr int ATS = 36;                       // ATT row stride (floats)
constexpr int HS = 68;                        // HID row stride (floats)
constexpr int KV_F = SJ * SH * SEQ * 4;       // 8704 floats each
constexpr int SPT3_RING_BYTES = (ROWS * XS + 2 * KV_F + ROWS * ATS) * 4;   // 147968: X | K | V | ATT
constexpr int SPT3_LDS_BYTES = 160 * 1024;          // + 15872 B: staged weights of the next phase | parameter vectors
// Weights and parameter vectors of a phase are staged in LDS while the phase BEFORE it runs (LDS-DMA for the packed
// weights, one float4 per thread for the 456 epilogue values of a block): a phase that starts with ~16 global
// loads per lane waits ~1.5 k cycles for L2 before its first MFMA, five times per block application (14 % of the kernel).
//   S_W   spare + 0      8 KiB   proj weights (4 KiB, staged during qkv + attention), then fc2 weights (staged during fc1)
//   S_PAR spare + 8 KiB  2 x 456 floats, double buffered by block application (staged during fc2 of the one before)
//   F1    K + 0          8 KiB   fc1 weights (staged during proj: K is dead after the attention); HID starts 12 KiB in
//   Q     ATT + 20 KiB   12 KiB  qkv weights of the NEXT application (staged during fc2; HID ends at ATT + 16.3 KiB)
constexpr int SPT3_HID_OFF = 3072;                  // floats: HID = K + 12 KiB
constexpr int SPT3_Q_OFF = 20480;                   // bytes into ATT
static_assert(SPT3_HID_OFF + ROWS * HS <= 2 * KV_F + ROWS * ATS, "HID does not fit its alias");
static_assert((SPT3_HID_OFF + ROWS * HS - 2 * KV_F) * 4 <= SPT3_Q_OFF, "HID reaches into the staged qkv weights");
static_assert(SPT3_Q_OFF + 12 * 1024 <= ROWS * ATS * 4, "staged qkv weights do not fit behind HID in ATT");
static_assert(SPT3_RING_BYTES + 8 * 1024 + 2 * SPT3_NPAR * 4 <= SPT3_LDS_BYTES, "spare LDS too small");

typedef float f32x2 __attribute__((ext_vector_type(2)));

// largest power of two p with p * v <= 2^15 (v > 0, finite); 1 for v == 0
__device__ inline float spt_window_scale(float v) {
    if (!(v > 0.f) || !(v < 3.0e38f)) return 1.0f;
    int e;
    (void)frexpf(32768.0f / v, &e);
    e = e - 1 < -100 ? -100 : (e - 1 > 100 ? 100 : e - 1);
    return ldexpf(1.0f, e);
}

// The D = 32 Linear layers of an SPT block as split-operand fp16 GEMMs (the arithmetic of h2_gemm.hip: x = hi + lo, three
// products, exact power-of-two scales): ONE workgroup packs a block.
//   * LayerNorm GEMMs (qkv, fc1): gamma is folded into W, beta and the bias into c_n = b_n + sum_k beta_k W_nk; the kernel
//     multiplies z = (x - mean) rstd 2^10;
//   * every column n has its own scale sw_n (max_k |W'_nk| sw_n in [2^13, 2^14)) that the epilogue multiplier sc_n takes out;
//   * the inputs of proj (attention output) and fc2 (GELU output) carry ONE static scale each from the data-free bound
//     |LN(x) . W'_n + c_n| <= sqrt(32) |W'_n|_2 + |c_n| of the producing columns (v columns of qkv; fc1), window 2^15;
//   * the q columns also carry hd^-0.5 log2 e (the scores are formed in the exp2 domain).
// Layout: spt_pack.hpp.
__global__ __launch_bounds__(256) void spt_pack_kernel(const float* __restrict__ qkv_w, const float* __restrict__ qkv_b,
                                                        const float* __restrict__ ln1_w, const float* __restrict__ ln1_b,
                                                        const float* __restrict__ proj_w, const float* __restrict__ proj_b,
                                                        const float* __restrict__ fc1_w, const float* __restrict__ fc1_b,
                                                        const float* __restrict__ ln2_w, const float* __restrict__ ln2_b,
                                                        const float* __restrict__ fc2_w, const float* __restrict__ fc2_b,
                                                        char* __restrict__ dst, int fold_q) {
    __shared__ float Wf[8192];                  // qkv' [96][32] | proj [32][32] | fc1' [64][32] | fc2 [32][64]
    __shared__ float cn[SPT_NCOL], sw[SPT_NCOL], bnd[SPT_NCOL], scal[2];
    const int tid = threadIdx.x;
    for (int i = tid; i < 8192; i += 256) {
        float w;
        if (i < 3072) w = qkv_w[i] * ln1_w[i & 31];
        else if (i < 4096) w = proj_w[i - 3072];
        else if (i < 6144) w = fc1_w[i - 4096] * ln2_w[i & 31];
        else w = fc2_w[i - 6144];
        Wf[i] = w;
    }
    __syncthreads();
    if (tid < SPT_NCOL) {
        const int n = tid;
        const float *wr, *raw, *beta = nullptr;
        int K = 32;
        float bias;
        if (n < 96) { wr = Wf + n * 32; raw = qkv_w + n * 32; beta = ln1_b; bias = qkv_b[n]; }
        else if (n < 128) { wr = Wf + 3072 + (n - 96) * 32; raw = proj_w + (n - 96) * 32; bias = proj_b[n - 96]; }
        else if (n < 192) { wr = Wf + 4096 + (n - 128) * 32; raw = fc1_w + (n - 128) * 32; beta = ln2_b; bias = fc1_b[n - 128]; }
        else { wr = Wf + 6144 + (n - 192) * 64; raw = fc2_w + (n - 192) * 64; bias = fc2_b[n - 192]; K = 64; }
        float amax = 0.f;
        double ss = 0.0, c = (double)bias;
        for (int k = 0; k < K; ++k) {
            amax = fmaxf(amax, fabsf(wr[k]));
            ss += (double)wr[k] * (double)wr[k];
            if (beta) c += (double)raw[k] * (double)beta[k];
        }
        float s = 1.0f;
        if (amax > 0.f && amax < 3.0e38f) {
            int e;
            (void)frexpf(amax, &e);             // amax = m 2^e, m in [0.5, 1): amax 2^(14 - e) in [2^13, 2^14)
            e = 14 - e;
            e = e < -100 ? -100 : (e > 100 ? 100 : e);
            s = ldexpf(1.0f, e);
        }
        cn[n] = (float)c;
        sw[n] = s;
        bnd[n] = beta ? (float)(sqrt(32.0) * sqrt(ss)) + fabsf((float)c) : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        float batt = 0.f, bhid = 0.f;
        for (int n = 64; n < 96; ++n) batt = fmaxf(batt, bnd[n]);                    // v columns of qkv
        for (int n = SPT_C_FC1; n < SPT_C_FC2; ++n) bhid = fmaxf(bhid, bnd[n]);
        scal[0] = spt_window_scale(batt);
        scal[1] = spt_window_scale(bhid);
    }
    __syncthreads();
    float* vec = reinterpret_cast<float*>(dst + SPT_PACK_VEC);
    if (tid < SPT_NCOL) {
        const int n = tid;
        float c = cn[n], sc;
        if (n < 96) sc = 1.0f / (SPT_SA * sw[n]);
        else if (n < 128) sc = 1.0f / (scal[0] * sw[n]);
        else if (n < 192) sc = 1.0f / (SPT_SA * sw[n]);
        else sc = 1.0f / (scal[1] * sw[n]);
        if (n < 32 && fold_q) { c *= SPT_QS; sc *= SPT_QS; }
        vec[n] = c;
        vec[SPT_NCOL + n] = sc;
    }
    if (tid < 8) vec[2 * SPT_NCOL + tid] = tid == 0 ? scal[0] : (tid == 1 ? 0.5f * scal[1] : 0.f);
    // fragment f of the packed block = 8 consecutive k of one weight row (scaled by its column scale), two parts
    sf16x8* frag = reinterpret_cast<sf16x8*>(dst);
    for (int idx = tid; idx < 16 * 64; idx += 256) {
        const int lane = idx & 63, u = idx >> 6, li = lane & 15, kq = lane >> 4;
        const float* src;
        int n;
        if (u < 6) { n = 16 * u + li; src = Wf + n * 32 + 8 * kq; }
        else if (u < 8) { n = 16 * (u - 6) + li; src = Wf + 3072 + n * 32 + 8 * kq; n += SPT_C_PROJ; }
        else if (u < 12) { n = 16 * (u - 8) + li; src = Wf + 4096 + n * 32 + 8 * kq; n += SPT_C_FC1; }
        else { n = 16 * ((u - 12) >> 1) + li; src = Wf + 6144 + n * 64 + 32 * ((u - 12) & 1) + 8 * kq; n += SPT_C_FC2; }   // [n][ks]
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = src[j] * sw[n];
        sf16x8 hi, lo;
        spt_split2(x, hi, lo);
        frag[(size_t)(u * 2) * 64 + lane] = hi;
        frag[(size_t)(u * 2 + 1) * 64 + lane] = lo;
    }
}

// fold_q: the q columns carry hd^-0.5 log2 e (the SPT kernel's exp2-domain attention); 0 for the D = 32 FPT blocks, whose
// attention kernel scales q itself
int launch_spt_pack(const mpl_block_weights* bw_host, unsigned short* dst, int fold_q, hipStream_t s) {
    const mpl_block_weights* b = bw_host;
    if (!b || !dst || !b->qkv_w || !b->proj_w || !b->fc1_w || !b->fc2_w || !b->qkv_b || !b->proj_b || !b->fc1_b || !b->fc2_b ||
        !b->ln1_w || !b->ln1_b || !b->ln2_w || !b->ln2_b)
        return MPL_E_INVALID;
    ProfScope prof(MPL_K_PACK, s);
    hipLaunchKernelGGL(spt_pack_kernel, dim3(1), dim3(256), 0, s, b->qkv_w, b->qkv_b, b->ln1_w, b->ln1_b, b->proj_w, b->proj_b, b->fc1_w,
                       b->fc1_b, b->ln2_w, b->ln2_b, b->fc2_w, b->fc2_b, reinterpret_cast<char*>(dst), fold_q);
    return hip_check_launch();
}

size_t spt_pack_bytes() { return SPT_PACK_BYTES; }

template <int N>
struct SptInt { static constexpr int value = N; };

// One Linear phase of ONE wave as straight-line code: the wave's units u = NCT m + n (row tile m, column tile n) of the phase's
// (m, n) list are LO .. HI - 1, compile-time (SPT_BY_WAVE below: one instantiation per wave of the workgroup), so every row tile,
// column range and LDS offset is a constant and nothing is left of the unit loop.  KS k steps of 32 (fc2: 2); LN: the A fragment
// is the normalised row of X (qkv's ln_frag), else a plain operand row (stride AST) that already carries its static scale; GELU:
// D = gelu(y) times the scale of the fc2 operand (stride DST), else the residual D += y.  An A fragment is formed once per row
// tile the wave touches; the operand rows -- and the residual rows -- of the NEXT row tile are read before the products of this
// one.  The product chain of a unit is mfma3 per k step, one unit after the other: chains of neighbouring column tiles
// interleaved product by product in the SOURCE gave other bits in the 4-sequence form on the device (HISTORY.md), so the order
// among independent chains is left to the compiler.
template <int KS, bool LN, bool GELU, int NCT, int AST, int DST, int LO, int HI>
__device__ __forceinline__ void spt_linear_role(const float* A, float* D, const char* wsec, const float* par, int col0, float hs,
                                                int lane) {
    if constexpr (HI > LO) {
        constexpr int M0 = LO / NCT, NM = (HI - 1) / NCT - M0 + 1;
        const int li = lane & 15, kq = lane >> 4;
        sf16x8 w[NCT][KS][2];
        float4 bc[NCT], sc[NCT];               // c_n and sc_n of this lane's columns
#pragma unroll
        for (int n = 0; n < NCT; ++n) {
            if (HI - LO < NCT && (n - LO % NCT + NCT) % NCT >= HI - LO) continue;     // a column tile this wave never meets
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) spt_load_unit(wsec, n * KS + ks, lane, w[n][ks]);
            bc[n] = ::mpl::ld4(par + col0 + 16 * n + 4 * kq);
            sc[n] = ::mpl::ld4(par + SPT_NCOL + col0 + 16 * n + 4 * kq);
        }
        const float* a0 = A + li * AST + 8 * kq;
        float* d0 = D + li * DST + 4 * kq;
        float4 raw[KS][2], res[NCT];
        auto read_tile = [&](int i) {          // operand rows and residual rows of the wave's i-th row tile
            const int m = M0 + i;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                raw[ks][0] = ::mpl::ld4(a0 + m * 16 * AST + 32 * ks);
                raw[ks][1] = ::mpl::ld4(a0 + m * 16 * AST + 32 * ks + 4);
            }
            if (!GELU) {
#pragma unroll
                for (int n = 0; n < NCT; ++n)
                    if (NCT * m + n >= LO && NCT * m + n < HI) res[n] = ::mpl::ld4(d0 + m * 16 * DST + 16 * n);
            }
        };
        read_tile(0);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int m = M0 + i;
            sf16x8 ah[KS], al[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (LN) {
                    spt_ln_split(raw[ks][0], raw[ks][1], ah[ks], al[ks]);
                } else {
                    const float4 x0 = raw[ks][0], x1 = raw[ks][1];
                    const float y[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                    spt_split2(y, ah[ks], al[ks]);
                }
            }
            float4 x[NCT];
#pragma unroll
            for (int n = 0; n < NCT; ++n) x[n] = res[n];
            if (i + 1 < NM) read_tile(i + 1);
            f32x4 c[NCT];
#pragma unroll
            for (int n = 0; n < NCT; ++n) c[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int n = 0; n < NCT; ++n) {
                if (NCT * m + n < LO || NCT * m + n >= HI) continue;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) c[n] = mfma3(w[n][ks], ah[ks], al[ks], c[n]);
            }
#pragma unroll
            for (int n = 0; n < NCT; ++n) {
                if (NCT * m + n < LO || NCT * m + n >= HI) continue;
                float* dd = d0 + m * 16 * DST + 16 * n;
                if (GELU)
                    st4(dd, float4{gelu_as_scaled(fmaf(c[n][0], sc[n].x, bc[n].x), hs), gelu_as_scaled(fmaf(c[n][1], sc[n].y, bc[n].y), hs),
                                   gelu_as_scaled(fmaf(c[n][2], sc[n].z, bc[n].z), hs), gelu_as_scaled(fmaf(c[n][3], sc[n].w, bc[n].w), hs)});
                else
                    st4(dd, float4{x[n].x + fmaf(c[n][0], sc[n].x, bc[n].x), x[n].y + fmaf(c[n][1], sc[n].y, bc[n].y),
                                   x[n].z + fmaf(c[n][2], sc[n].z, bc[n].z), x[n].w + fmaf(c[n][3], sc[n].w, bc[n].w)});
            }
        }
    }
}
// the phase of wave `wv` (scalar): units NU * wv / NWAVE .. NU * (wv + 1) / NWAVE - 1 of the NU = MTS * NCT of the workgroup
#define SPT_ROLE(W, MTS, KS, LN, GELU, NCT, AST, DST, ...) \
    spt_linear_role<KS, LN, GELU, NCT, AST, DST, ((MTS) * (NCT) * (W)) / NWAVE, ((MTS) * (NCT) * ((W) + 1)) / NWAVE>(__VA_ARGS__)
#define SPT_BY_WAVE(wv, ...)                          \
    switch (wv) {                                     \
        case 0: SPT_ROLE(0, __VA_ARGS__); break;      \
        case 1: SPT_ROLE(1, __VA_ARGS__); break;      \
        case 2: SPT_ROLE(2, __VA_ARGS__); break;      \
        case 3: SPT_ROLE(3, __VA_ARGS__); break;      \
        case 4: SPT_ROLE(4, __VA_ARGS__); break;      \
        case 5: SPT_ROLE(5, __VA_ARGS__); break;      \
        case 6: SPT_ROLE(6, __VA_ARGS__); break;      \
        default: SPT_ROLE(7, __VA_ARGS__); break;     \
    }


// SS = sequences per workgroup (16, 8, 4, 2 or 1): rows = joint * SS + sequence, 17 SS of them in MTS row tiles.  A launch of few
// sequences takes as few per workgroup as keep it within one workgroup per CU (launch_spt): the kernel's time is VALU work per ROW
// TILE, so 4 sequences per workgroup walk 5 tiles instead of 17.  The arithmetic of a row does not depend on SS (the matrix
// instructions treat rows independently; the attention of a (sequence, head, query joint) visits the keys in the same order).
template <int SS>
__global__ __launch_bounds__(NTHR, 1) void spt3_kernel(const SptParams p) {
    constexpr int RLIVE = SJ * SS;                 // live rows
    constexpr int MTS = (RLIVE + 15) / 16;         // row tiles
    constexpr int NT = (MTS + 3) / 4;              // row tiles of a wave in the qkv / attention phases (tiles part, part + 4, ...)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X = smem;
    float* Kb = smem + ROWS * XS;
    float* Vb = Kb + KV_F;
    float* ATT = Vb + KV_F;
    float* HID = Kb + SPT3_HID_OFF;                // alias (K, V, ATT are dead between proj and the next qkv)
    char* S_W = reinterpret_cast<char*>(ATT + ROWS * ATS);
    float* S_PAR = reinterpret_cast<float*>(S_W + 8 * 1024);
    char* R_F1 = reinterpret_cast<char*>(Kb);
    char* R_Q = reinterpret_cast<char*>(ATT) + SPT3_Q_OFF;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;      // li = sequence (row in tile), kq = k quarter / column quad
    // every barrier of this kernel also publishes staged DMA pieces: the compiler does not see the LDS-DMA requests (inline
    // asm), so the wait for them is explicit
    auto phase_sync = [&]() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    const int hg = wave & 1, part = wave >> 1;     // head group, joint class
    const int view = blockIdx.x % p.V;
    const int b0 = (blockIdx.x / p.V) * SS;
    const int sl = li % SS;                        // this lane's sequence in every row tile (16 is a multiple of SS)
    const mpl_spt_set set = p.sets[(p.flags & MPL_F_MULTI_SPT) ? view : 0];
    const float* pose = p.poses[view];
    const float* ray = p.rays[view];
    const float* cen = p.centers[view];

    // stage n_pieces KiB of a packed block (section at byte_off) into LDS at dst: wave w brings pieces w, w + 8, ...;
    // the __syncthreads() that ends the current phase (it waits for vmcnt(0)) publishes them
    auto stage_w = [&](char* dst, const unsigned short* pack, int byte_off, int n_pieces) {
        const unsigned l0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)dst;
        for (int i = wave; i < n_pieces; i += NWAVE)
            ::mpl::dma16(reinterpret_cast<const float*>(reinterpret_cast<const char*>(pack) + byte_off + i * 1024) + lane * 4,
                         l0 + (unsigned)(i * 1024));
    };
    // the epilogue vectors of a block (c | sc | scalars, written by mpl_spt_pack behind the fragments), one float4 per thread
    auto load_par = [&](const mpl_block_weights& b) -> float4 {
        if (tid >= SPT3_NPAR / 4) return float4{0.f, 0.f, 0.f, 0.f};
        return ld4(G(reinterpret_cast<const float*>(reinterpret_cast<const char*>(b.qkv_w3) + SPT_PACK_VEC)) + 4 * tid);
    };
    auto store_par = [&](int app_of, const float4& v) {
        if (tid < SPT3_NPAR / 4) st4(S_PAR + (app_of & 1) * SPT3_NPAR + 4 * tid, v);
    };
    mpl_block_weights bw;
    if (p.n_apps > 0) {                            // application 0: its qkv weights and parameters, under the embedding
        bw = set.blocks[p.sched[0] & 0x7f];
        stage_w(R_Q, bw.qkv_w3, SPT_PACK_QKV, 12);
    }
    const float4 par0 = p.n_apps > 0 ? load_par(bw) : float4{0.f, 0.f, 0.f, 0.f};
    spt_embed<true, SS>(p, set, X, tid, b0, pose, ray, cen, SS, MTS * 16);
    store_par(0, par0);
    phase_sync();

    auto load_w = [&](const char* region, int unit, sf16x8 (&w)[2]) { spt_load_unit(region, unit, lane, w); };   // from the staged section in LDS
    // normalised, split A fragment of row tile m (K = 32): lane (s, kq) holds k = 8 kq .. 8 kq + 7 of row 16 m + s
    auto ln_frag = [&](int m, sf16x8& ah, sf16x8& al) {
        const float* xr = X + (m * 16 + li) * XS + 8 * kq;
        spt_ln_split(::mpl::ld4(xr), ::mpl::ld4(xr + 4), ah, al);
    };
    for (int app = 0; app < p.n_apps; ++app) {
        const bool weighted = (p.sched[app] & 0x80) != 0;
        bw = set.blocks[p.sched[app] & 0x7f];
        const unsigned short* pack = bw.qkv_w3;
        const float* par = S_PAR + (app & 1) * SPT3_NPAR;
        stage_w(S_W, pack, SPT_PACK_PROJ, 4);      // proj weights: land during qkv + attention
        // ---------------- qkv: this wave's q, k, v tiles (head group hg) of its joints
        {
            sf16x8 wq[3][2];
            float4 bq[3], sq[3];                   // c_n and sc_n of this lane's q, k, v columns (q: times hd^-0.5 log2 e)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                load_w(R_Q, 2 * c + hg, wq[c]);
                bq[c] = ::mpl::ld4(par + SPT_C_QKV + 32 * c + 16 * hg + 4 * kq);
                sq[c] = ::mpl::ld4(par + SPT_NCOL + SPT_C_QKV + 32 * c + 16 * hg + 4 * kq);
            }
            float4 q[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                q[t] = float4{0.f, 0.f, 0.f, 0.f};
                if (part + 4 * t < MTS && !(p.abl & 8)) {
                    const int m = part + 4 * t;
                    const int j = (16 * m + li) / SS;                   // this lane's joint in row tile m (SS = 16: j = m)
                    const bool live = 16 * m + li < RLIVE;
                    sf16x8 ah, al;
                    ln_frag(m, ah, al);
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                    const f32x4 cq = mfma3(wq[0], ah, al, z), ck = mfma3(wq[1], ah, al, z), cv = mfma3(wq[2], ah, al, z);
                    q[t] = float4{fmaf(cq[0], sq[0].x, bq[0].x), fmaf(cq[1], sq[0].y, bq[0].y), fmaf(cq[2], sq[0].z, bq[0].z),
                                  fmaf(cq[3], sq[0].w, bq[0].w)};
                    const int h = 4 * hg + kq;
                    // K tile: keys in PAIRS, components interleaved -- [pair][plane][h][seq]{c_j, c_j+1, c'_j, c'_j+1} with plane 0
                    // = (x, y), plane 1 = (z, w) -- so that two scores come out of one packed multiply-add; the 17th key stays
                    // a plain [h][seq]{x, y, z, w} record behind the 8 pairs
                    const float kx = fmaf(ck[0], sq[1].x, bq[1].x), ky = fmaf(ck[1], sq[1].y, bq[1].y);
                    const float kz = fmaf(ck[2], sq[1].z, bq[1].z), kw = fmaf(ck[3], sq[1].w, bq[1].w);
                    if (live && j < SJ - 1) {
                        float* kp = Kb + ((((j >> 1) * 2) * SH + h) * SS + sl) * 4 + (j & 1);
                        kp[0] = kx;
                        kp[2] = ky;
                        kp[SH * SS * 4] = kz;
                        kp[SH * SS * 4 + 2] = kw;
                    } else if (live) {
                        st4(Kb + (SJ - 1) * SH * SS * 4 + (h * SS + sl) * 4, float4{kx, ky, kz, kw});
                    }
                    if (live)
                        st4(Vb + ((j * SH + h) * SS + sl) * 4, float4{fmaf(cv[0], sq[2].x, bq[2].x), fmaf(cv[1], sq[2].y, bq[2].y),
                                                                       fmaf(cv[2], sq[2].z, bq[2].z), fmaf(cv[3], sq[2].w, bq[2].w)});
                }
            }
            phase_sync();
            // ---------------- attention (:55-64): lane = (sequence li, head h), its <= 5 query joints against all 17 keys.
            // Scores in the exp2 domain (the q columns carry hd^-0.5 log2 e = 0.5 log2 e from their epilogue multiplier), the
            // probabilities stay unnormalised until the output row is complete; the output leaves with the static scale of the
            // proj operand (par[448], a power of two).
            // A wave whose last tile part + 4 (NT - 1) does not exist (SS = 16: every part but 0) runs the phase over NT - 1 tiles.
            auto attention = [&](auto live_tiles) {
                constexpr int NL = decltype(live_tiles)::value;
                const int h = 4 * hg + kq;
                float sc[NL][SJ];
#pragma unroll
                for (int jp = 0; jp < SJ / 2; ++jp) {
                    const float4 k01 = ::mpl::ld4(Kb + (((jp * 2) * SH + h) * SS + sl) * 4);        // x_j x_j+1 y_j y_j+1
                    const float4 k23 = ::mpl::ld4(Kb + (((jp * 2 + 1) * SH + h) * SS + sl) * 4);    // z_j z_j+1 w_j w_j+1
                    const f32x2 kx = {k01.x, k01.y}, ky = {k01.z, k01.w}, kz = {k23.x, k23.y}, kw = {k23.z, k23.w};
#pragma unroll
                    for (int t = 0; t < NL; ++t) {
                        const f32x2 qx = {q[t].x, q[t].x}, qy = {q[t].y, q[t].y}, qz = {q[t].z, q[t].z}, qw = {q[t].w, q[t].w};
                        f32x2 s2 = qx * kx;
                        s2 = __builtin_elementwise_fma(qy, ky, s2);
                        s2 = __builtin_elementwise_fma(qz, kz, s2);
                        s2 = __builtin_elementwise_fma(qw, kw, s2);
                        sc[t][2 * jp] = s2[0];
                        sc[t][2 * jp + 1] = s2[1];
                    }
                }
                {
                    const float4 k = ::mpl::ld4(Kb + (SJ - 1) * SH * SS * 4 + (h * SS + sl) * 4);
#pragma unroll
                    for (int t = 0; t < NL; ++t)
                        sc[t][SJ - 1] = fmaf(q[t].w, k.w, fmaf(q[t].z, k.z, fmaf(q[t].y, k.y, q[t].x * k.x)));
                }
                const float s_att = par[2 * SPT_NCOL];
                // Confidence of this lane's row in tile t = 0 (the weighted application scales the query rows by it), rebuilt
                // from the lane index where it is needed: as a loop invariant the address -- one per tile, as it was written
                // before -- is kept in registers across every phase of every application, which the 16-sequence form paid for
                // with scratch.  The empty asm makes the lane index a value of this iteration.
                const float* conf0 = nullptr;
                if (weighted) {
                    int l16 = li;
                    asm volatile("" : "+v"(l16));
                    conf0 = pose + ((size_t)(b0 + l16 % SS) * SJ + (16 * part + l16) / SS) * 3 + 2;
                }
                float inv[NL];
#pragma unroll
                for (int t = 0; t < NL; ++t) {
                    float mx = sc[t][0];
#pragma unroll
                    for (int j = 1; j < SJ; ++j) mx = fmaxf(mx, sc[t][j]);
                    float l = 0.f;
#pragma unroll
                    for (int j = 0; j < SJ; ++j) {
                        sc[t][j] = __builtin_amdgcn_exp2f(sc[t][j] - mx);
                        l += sc[t][j];
                    }
                    inv[t] = __builtin_amdgcn_rcpf(l) * s_att;              // v_rcp_f32 (1 ulp)
                    if (weighted) {  // attn * conf_weights.unsqueeze(1) after softmax (:61-62): scales the query row
                        // row r = 16 (part + 4 t) + li is joint r / SS = (16 part + li) / SS + (64 / SS) t: a constant offset per tile
                        const int b = b0 + sl, r = 16 * (part + 4 * t) + li;
                        inv[t] *= (b < p.B && r < RLIVE) ? conf0[3 * (64 / SS) * t] : 0.f;
                    }
                }
                float4 o[NL];
#pragma unroll
                for (int t = 0; t < NL; ++t) o[t] = float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < SJ; ++j) {
                    const float4 v = ::mpl::ld4(Vb + ((j * SH + h) * SS + sl) * 4);
#pragma unroll
                    for (int t = 0; t < NL; ++t) {
                        const float pj = sc[t][j];
                        o[t].x = fmaf(pj, v.x, o[t].x);
                        o[t].y = fmaf(pj, v.y, o[t].y);
                        o[t].z = fmaf(pj, v.z, o[t].z);
                        o[t].w = fmaf(pj, v.w, o[t].w);
                    }
                }
#pragma unroll
                for (int t = 0; t < NL; ++t) {
                    o[t] = float4{o[t].x * inv[t], o[t].y * inv[t], o[t].z * inv[t], o[t].w * inv[t]};
                    // the confidence weights are data (reference :61-62 multiplies the softmax rows by whatever `conf` it is
                    // given): only with them can the operand leave the window its static, data-free scale assumes.  That is
                    // reported, never absorbed: the row becomes NaN (so do the poses of its sequence) and the device error word
                    // gets bit 1 (value 2) -- the next API call and check_device() raise, pointing at the native-fp32 engine, which has
                    // no window.  (Rounds 3-5 clamped to +-65000 here: plausible-looking poses from saturated operands.)
                    // The report is for a FINITE operand beyond the window.  A row that is NaN or infinite comes from a NaN or
                    // infinite keypoint or confidence, the caller's data, which the reference answers with NaN poses for that
                    // sequence: the row becomes NaN all the same, nothing saturated is hidden, and the error word stays clear.
                    // (fmaxf drops a NaN operand, so `big` is NaN only when all four components are; a non-finite confidence
                    // makes inv[t], a non-finite keypoint every q / k / v of the sequence non-finite, so a row never mixes a NaN
                    // component with a finite one beyond the window.)
                    if (weighted) {
                        const float big = fmaxf(fmaxf(fabsf(o[t].x), fabsf(o[t].y)), fmaxf(fabsf(o[t].z), fabsf(o[t].w)));
                        if (!(big <= 65000.f)) {
                            const float qn = __builtin_nanf("");
                            o[t] = float4{qn, qn, qn, qn};
                            if (big < __builtin_inff() && p.err_host)
                                __hip_atomic_fetch_or(p.err_host, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < NL; ++t) st4(ATT + ((part + 4 * t) * 16 + li) * ATS + 4 * h, o[t]);
            };
            if (!(p.abl & 1)) {
                if (part + 4 * (NT - 1) < MTS) attention(SptInt<NT>{});
                else if (NT > 1) attention(SptInt<(NT > 1 ? NT - 1 : 1)>{});
            }
        }
        phase_sync();
        // ---------------- X += attn_out . Wproj^T + b : 17 x 2 tiles, dealt as contiguous ranges of the (m, n) list
        stage_w(R_F1, pack, SPT_PACK_FC1, 8);           // fc1 weights into the dead K tile
        if (!(p.abl & 32)) SPT_BY_WAVE(wave, MTS, 1, false, false, 2, ATS, XS, ATT, X, S_W, par, SPT_C_PROJ, 0.f, lane);
        phase_sync();
        // ---------------- Hid = gelu(LN2(X) . W1^T + b) : 17 x 4 tiles; par[449] = half the static scale of the fc2 operand
        stage_w(S_W, pack, SPT_PACK_FC2, 8);            // fc2 weights (the proj weights in S_W were read a phase ago)
        if (!(p.abl & 64))
            SPT_BY_WAVE(wave, MTS, 1, true, true, 4, XS, HS, X, HID, R_F1, par, SPT_C_FC1, par[2 * SPT_NCOL + 1], lane);
        phase_sync();
        // ---------------- X += Hid . W2^T + b : K = 64 (two k steps), 17 x 2 tiles
        {
            // the next application's qkv weights (behind HID in ATT) and parameters travel under this phase
            float4 parn = float4{0.f, 0.f, 0.f, 0.f};
            if (app + 1 < p.n_apps) {
                const mpl_block_weights bn = set.blocks[p.sched[app + 1] & 0x7f];
                stage_w(R_Q, bn.qkv_w3, SPT_PACK_QKV, 12);
                parn = load_par(bn);
            }
            if (!(p.abl & 128)) SPT_BY_WAVE(wave, MTS, 2, false, false, 2, HS, XS, HID, X, S_W, par, SPT_C_FC2, 0.f, lane);
            if (app + 1 < p.n_apps) store_par(app + 1, parn);
        }
        phase_sync();
    }
    spt_epilogue<true, SS>(p, X, tid, view, b0, pose, ray, cen, SS, MTS * 16);
}

// the LDS opt-in (>64 KiB of dynamic LDS, once per device) and the launch of one SS
template <int SS>
static int launch_spt3(const SptParams& p, int grid, hipStream_t s) {
    if (int rc = kernel_lds_once<spt3_kernel<SS>>(SPT3_LDS_BYTES)) return rc;
    hipLaunchKernelGGL(spt3_kernel<SS>, dim3(grid), dim3(NTHR), SPT3_LDS_BYTES, s, p);
    return hip_check_launch();
}

int launch_spt_packed(const SptParams& p, int ss, int grid, hipStream_t s) {
    switch (ss) {
        case 1: return launch_spt3<1>(p, grid, s);
        case 2: return launch_spt3<2>(p, grid, s);
        case 4: return launch_spt3<4>(p, grid, s);
        case 8: return launch_spt3<8>(p, grid, s);
        case 16: return launch_spt3<16>(p, grid, s);
        default: return MPL_E_INVALID;
    }
}

}  // namespace mpl
