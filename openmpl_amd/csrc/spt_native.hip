// The SPT stage with every Linear on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), reading the reference's nn.Linear weights
// in place -- what precision "fp32_mfma" runs, and every model whose blocks carry no packed operand (spt.hip: spt_form ->
// MPL_SPT_STAGED / MPL_SPT_FRAGS).  spt_kernel<STAGED>, 512 threads = 8 waves, rows sequence-major (row = sequence * 17 + joint):
//   * A fragments come from LDS with one ds_read_b128 per 16-deep k step (k permuted identically on both operands); LayerNorm
//     is fused into their formation: the 32 values of a row sit in the 4 lanes {i, i+16, i+32, i+48}, two lane swaps per sum;
//   * attention (17 x 17 scores, head dim 4) is VALU work: one thread per (row, head), scores in registers, softmax without
//     any cross-lane traffic; k / v rows are LDS broadcasts.
// The two forms differ ONLY in where the weight fragments of a phase come from (FragWeights / StagedWeights below); each of the
// four Linear phases is written once (linear_phase), so a row is the same instruction sequence in both.
//   STAGED = false (9 .. 16 sequences): registers, loaded from global memory one phase ahead.  LDS: X[272][36] | Q[272][100].
//   STAGED = true  (1 .. 8 sequences):  a copy of the block in LDS, by LDS-DMA one application ahead -- a phase over 2-9 row tiles is
//                  SHORTER than the trip to L2 / HBM (2 us per phase with the other scheme).  LDS: WB[2][8704] | X[144][36] | Q[144][100].
// Q holds q | k | v in columns 0..95; the attention output overwrites q in place; the MLP hidden layer (64 wide) aliases q | k.
// Both maps are 147968 B: one workgroup per CU.
#include <type_traits>

#include "spt_stage.hpp"

namespace mpl {

constexpr int QS = 100;         // Q row stride (floats)
constexpr int SPT_LDS_BYTES = (ROWS * XS + ROWS * QS) * 4;  // 147968

// bench-only ablation mask (-DMPL_LAB builds of this file): 0 in the product, where everything it guards compiles away
__device__ __forceinline__ int spt_abl(const SptParams& p) {
#ifdef MPL_LAB
    return p.abl;
#else
    return 0;
#endif
}

// LayerNorm'ed A fragments of row tile m for a K = 32 GEMM: a0 covers k = 4kq..4kq+3, a1 k = 16+4kq..
__device__ __forceinline__ void ln_frags(const float* X, int m, int li, int kq, const float4& g0, const float4& g1,
                                         const float4& b0, const float4& b1, float4& a0, float4& a1) {
    const float* xr = X + (m * 16 + li) * XS + 4 * kq;
    float4 x0 = ld4(xr), x1 = ld4(xr + 16);
    float s = ((x0.x + x0.y) + (x0.z + x0.w)) + ((x1.x + x1.y) + (x1.z + x1.w));
    s = xor16_add(s);
    s = xor32_add(s);
    const float mean = s * (1.0f / 32.0f);
    x0.x -= mean; x0.y -= mean; x0.z -= mean; x0.w -= mean;
    x1.x -= mean; x1.y -= mean; x1.z -= mean; x1.w -= mean;
    float ss = ((x0.x * x0.x + x0.y * x0.y) + (x0.z * x0.z + x0.w * x0.w)) +
               ((x1.x * x1.x + x1.y * x1.y) + (x1.z * x1.z + x1.w * x1.w));
    ss = xor16_add(ss);
    ss = xor32_add(ss);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / 32.0f) + 1e-6f);
    a0.x = x0.x * rstd * g0.x + b0.x; a0.y = x0.y * rstd * g0.y + b0.y;
    a0.z = x0.z * rstd * g0.z + b0.z; a0.w = x0.w * rstd * g0.w + b0.w;
    a1.x = x1.x * rstd * g1.x + b1.x; a1.y = x1.y * rstd * g1.y + b1.y;
    a1.z = x1.z * rstd * g1.z + b1.z; a1.w = x1.w * rstd * g1.w + b1.w;
}

// All MFMA B fragments and LayerNorm / bias vectors of one Block that this lane needs (128 + 30 registers), loaded straight
// from the reference's [out][in] tensors.
struct BlockFrags {
    float4 wq[6][2]; float bq[6];     // attn.qkv: 6 column tiles x (k 0..15 | k 16..31)
    float4 wp[2][2]; float bp[2];     // attn.proj
    float4 w1[4][2]; float b1[4];     // mlp.fc1
    float4 w2[2][4]; float b2[2];     // mlp.fc2 (K = 64: four 16-deep steps)
    float4 g1a, g1b, e1a, e1b;        // norm1 gamma/beta of this lane's 8 k columns
    float4 g2a, g2b, e2a, e2b;        // norm2
};

// this lane's fragments of N column tiles x K 16-deep k steps of an [out][in] weight matrix of row length ldw, and their biases
template <int N, int K>
__device__ __forceinline__ void load_tiles(const float* w, const float* b, int ldw, float4 (&wf)[N][K], float (&bf)[N], int li, int kq) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const gfp wr = G(w) + (n * 16 + li) * ldw + 4 * kq;
#pragma unroll
        for (int q = 0; q < K; ++q) wf[n][q] = ld4(wr + 16 * q);
        bf[n] = G(b)[n * 16 + li];
    }
}
__device__ __forceinline__ void load_ln(const float* w, const float* b, float4& g0, float4& g1, float4& e0, float4& e1, int kq) {
    g0 = ld4(G(w) + 4 * kq); g1 = ld4(G(w) + 16 + 4 * kq);
    e0 = ld4(G(b) + 4 * kq); e1 = ld4(G(b) + 16 + 4 * kq);
}

// ---- the same fragments from a block STAGED in LDS (spt_kernel<true>: few sequences per workgroup).  A staged block is 32 1-KiB
// pieces in fragment order -- qkv: piece 2 n + h = W[16 n + li][16 h + 4 kq ..]; proj 12 + 2 n + h; fc1 16 + 2 n + h; fc2
// 24 + 4 n + q -- and, from float SPT_WB_VEC on, the vectors qkv_b[96] | proj_b[32] | fc1_b[64] | fc2_b[32] | ln1_w | ln1_b |
// ln2_w | ln2_b (32 each).
constexpr int SPT_WB_VEC = 8192;                 // floats
constexpr int SPT_WB_FLOATS = SPT_WB_VEC + 512;  // one staged block
constexpr int SPT_SMALL_ROWS = 144;              // token rows of the staged form: up to 8 sequences (136 rows) per workgroup
constexpr int SPT_SMALL_LDS_BYTES = (SPT_SMALL_ROWS * (XS + QS) + 2 * SPT_WB_FLOATS) * 4;   // 147968
// Staging is LDS-DMA with per-lane source addresses, pieces 0..31 weights, 32 / 33 the vectors; the waves w0 .. w0 + nw - 1 share them
// round robin.  What it costs is the rate at which the CU's address path accepts requests: ~60 cycles per piece in fragment order (16
// half-used lines; ~40 for a contiguous KiB), and a wave stands in its request until it is accepted -- 2100 cycles per wave and
// application when all eight waves request at the head of an application.  The requests are therefore made by the waves the attention
// phase leaves idle (17 nl x 8 (row, head) pairs: 136 threads at one sequence per workgroup).
__device__ __forceinline__ const float* spt_uniform(const float* q) {
    const unsigned long long v = (unsigned long long)(uintptr_t)q;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const float*>((uintptr_t)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ void stage_block(const mpl_block_weights& bwv, float* wb, int wave, int lane, int w0, int nw) {
    if (wave < w0 || wave >= w0 + nw) return;
    const int li = lane & 15, kq = lane >> 4;
    // The pointers came by vector loads: ALL of them into scalar registers first.  Left in vector registers the compiler puts a
    // vmcnt(0) in front of every use behind an opaque DMA statement -- i.e. waits for the previous piece's trip to memory, piece by piece.
    struct { const float *qkv_w, *proj_w, *fc1_w, *fc2_w, *qkv_b, *proj_b, *fc1_b, *fc2_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b; } bw;
    bw.qkv_w = spt_uniform(bwv.qkv_w); bw.proj_w = spt_uniform(bwv.proj_w); bw.fc1_w = spt_uniform(bwv.fc1_w); bw.fc2_w = spt_uniform(bwv.fc2_w);
    bw.qkv_b = spt_uniform(bwv.qkv_b); bw.proj_b = spt_uniform(bwv.proj_b); bw.fc1_b = spt_uniform(bwv.fc1_b); bw.fc2_b = spt_uniform(bwv.fc2_b);
    bw.ln1_w = spt_uniform(bwv.ln1_w); bw.ln1_b = spt_uniform(bwv.ln1_b); bw.ln2_w = spt_uniform(bwv.ln2_w); bw.ln2_b = spt_uniform(bwv.ln2_b);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)wb);
    for (int pc = wave - w0; pc < 34; pc += nw) {
        const float* src;
        bool on = true;
        if (pc < 12) src = bw.qkv_w + ((pc >> 1) * 16 + li) * SD + 16 * (pc & 1) + 4 * kq;
        else if (pc < 16) src = bw.proj_w + (((pc - 12) >> 1) * 16 + li) * SD + 16 * (pc & 1) + 4 * kq;
        else if (pc < 24) src = bw.fc1_w + (((pc - 16) >> 1) * 16 + li) * SD + 16 * (pc & 1) + 4 * kq;
        else if (pc < 32) src = bw.fc2_w + (((pc - 24) >> 2) * 16 + li) * (2 * SD) + 16 * (pc & 3) + 4 * kq;
        else if (pc == 32)
            src = lane < 24 ? bw.qkv_b + 4 * lane
                : lane < 32 ? bw.proj_b + 4 * (lane - 24)
                : lane < 48 ? bw.fc1_b + 4 * (lane - 32)
                : lane < 56 ? bw.fc2_b + 4 * (lane - 48) : bw.ln1_w + 4 * (lane - 56);
        else {
            src = lane < 8 ? bw.ln1_b + 4 * lane : lane < 16 ? bw.ln2_w + 4 * (lane - 8) : bw.ln2_b + 4 * (lane - 16);
            on = lane < 24;
        }
        if (on) dma16(src, lds0 + (unsigned)(pc * 1024));
    }
}
__device__ __forceinline__ float4 wb4(const float* wb, int piece, int lane) { return *reinterpret_cast<const float4*>(wb + piece * 256 + lane * 4); }
__device__ __forceinline__ float4 wbv4(const float* wb, int off, int kq) { return *reinterpret_cast<const float4*>(wb + SPT_WB_VEC + off + 4 * kq); }

// "Touch" prefetched fragments: an empty asm that reads them makes hipcc place their s_waitcnt HERE and not, together with the
// wait for loads issued a moment ago, in front of the first MFMA of the phase.
__device__ __forceinline__ void touch(const float4& a) {
    const f32x4 v = {a.x, a.y, a.z, a.w};
    asm volatile("" ::"v"(v));
}
__device__ __forceinline__ void touch(float a) { asm volatile("" ::"v"(a)); }

// one 16x16 output tile of a K = 32 GEMM: two independent accumulator chains (k 0..15 / 16..31) so that
// consecutive MFMAs never wait on the 40-cycle dependent-accumulator latency
__device__ __forceinline__ f32x4 tile_k32(const float4& a0, const float4& a1, const float4& w0, const float4& w1) {
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0;
    c0 = mfma16(a0.x, w0.x, c0); c1 = mfma16(a1.x, w1.x, c1);
    c0 = mfma16(a0.y, w0.y, c0); c1 = mfma16(a1.y, w1.y, c1);
    c0 = mfma16(a0.z, w0.z, c0); c1 = mfma16(a1.z, w1.z, c1);
    c0 = mfma16(a0.w, w0.w, c0); c1 = mfma16(a1.w, w1.w, c1);
    return c0 + c1;
}

// ---- the four Linear phases of a block application and where the staged block keeps their operands
enum { P_QKV = 0, P_PROJ = 1, P_FC1 = 2, P_FC2 = 3 };
template <int P>
struct Phase {
    static constexpr int NT = P == P_QKV ? 6 : P == P_FC1 ? 4 : 2;                            // column tiles of 16
    static constexpr int KH = P == P_FC2 ? 4 : 2;                                             // 16-deep k steps (K = 64 : 32)
    static constexpr int PIECE = P == P_QKV ? 0 : P == P_PROJ ? 12 : P == P_FC1 ? 16 : 24;    // staged: piece PIECE + KH n + q
    static constexpr int BIAS = P == P_QKV ? 0 : P == P_PROJ ? 96 : P == P_FC1 ? 128 : 192;   // staged: bias, floats from SPT_WB_VEC
    static constexpr int LN = P == P_QKV ? 224 : 288;       // staged: gamma | beta (32 each) of the LayerNorm in front of qkv / fc1
};

// The weight source of a form answers: the fragments and the bias of column tile n of phase P (tile; n is a compile-time index
// after unrolling), the LayerNorm vectors in front of P (ln), what the head of P does so that the NEXT operands arrive (begin).
// Fragment form: every phase first touches its own fragments (requested a phase ago, so the wait is free), then requests those of
// the next phase -- proj during qkv, fc1 during proj, fc2 during fc1, the next application's qkv during fc2 -- so each group has
// a whole phase to arrive and at most two groups are live at a time.
struct FragWeights {
    BlockFrags F;
    int li, kq;
    template <int P>
    __device__ __forceinline__ void tile(int n, float4 (&w)[Phase<P>::KH], float& b) const {
        if constexpr (P == P_QKV) { w[0] = F.wq[n][0]; w[1] = F.wq[n][1]; b = F.bq[n]; }
        else if constexpr (P == P_PROJ) { w[0] = F.wp[n][0]; w[1] = F.wp[n][1]; b = F.bp[n]; }
        else if constexpr (P == P_FC1) { w[0] = F.w1[n][0]; w[1] = F.w1[n][1]; b = F.b1[n]; }
        else { w[0] = F.w2[n][0]; w[1] = F.w2[n][1]; w[2] = F.w2[n][2]; w[3] = F.w2[n][3]; b = F.b2[n]; }
    }
    template <int P>
    __device__ __forceinline__ void ln(float4 (&g)[2], float4 (&e)[2]) const {
        if constexpr (P == P_QKV) { g[0] = F.g1a; g[1] = F.g1b; e[0] = F.e1a; e[1] = F.e1b; }
        else { g[0] = F.g2a; g[1] = F.g2b; e[0] = F.e2a; e[1] = F.e2b; }
    }
    template <int N, int K>
    static __device__ __forceinline__ void touch_all(const float4 (&w)[N][K], const float (&b)[N]) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
#pragma unroll
            for (int k = 0; k < K; ++k) touch(w[n][k]);
            touch(b[n]);
        }
    }
    template <int P>
    __device__ __forceinline__ void load(const mpl_block_weights& bw) {      // request the fragments of phase P
        if constexpr (P == P_QKV) { load_ln(bw.ln1_w, bw.ln1_b, F.g1a, F.g1b, F.e1a, F.e1b, kq); load_tiles(bw.qkv_w, bw.qkv_b, SD, F.wq, F.bq, li, kq); }
        else if constexpr (P == P_PROJ) load_tiles(bw.proj_w, bw.proj_b, SD, F.wp, F.bp, li, kq);
        else if constexpr (P == P_FC1) { load_ln(bw.ln2_w, bw.ln2_b, F.g2a, F.g2b, F.e2a, F.e2b, kq); load_tiles(bw.fc1_w, bw.fc1_b, SD, F.w1, F.b1, li, kq); }
        else load_tiles(bw.fc2_w, bw.fc2_b, 2 * SD, F.w2, F.b2, li, kq);
    }
    template <int P>
    __device__ __forceinline__ void begin(const mpl_block_weights& bw, const mpl_block_weights& bw_next, bool more) {
        if constexpr (P == P_QKV) { touch_all(F.wq, F.bq); touch(F.g1a); touch(F.g1b); touch(F.e1a); touch(F.e1b); }
        else if constexpr (P == P_PROJ) touch_all(F.wp, F.bp);
        else if constexpr (P == P_FC1) { touch_all(F.w1, F.b1); touch(F.g2a); touch(F.g2b); touch(F.e2a); touch(F.e2b); }
        else touch_all(F.w2, F.b2);
        if constexpr (P != P_FC2) load<P + 1>(bw);
        else if (more) load<P_QKV>(bw_next);     // the qkv fragments are long dead: the next application's weights
    }
};
// Staged form: the block of this application lies in LDS at wb (stage_block brought it an application ago; the kernel requests the
// next one between qkv and attention and awaits it in front of the application's last barrier).  Fragments are read ON DEMAND, tile
// by tile: a wave owns one or two output tiles of a phase.
struct StagedWeights {
    const float* wb;
    int lane, li, kq;
    template <int P>
    __device__ __forceinline__ void tile(int n, float4 (&w)[Phase<P>::KH], float& b) const {
#pragma unroll
        for (int q = 0; q < Phase<P>::KH; ++q) w[q] = wb4(wb, Phase<P>::PIECE + Phase<P>::KH * n + q, lane);
        b = wb[SPT_WB_VEC + Phase<P>::BIAS + n * 16 + li];
    }
    template <int P>
    __device__ __forceinline__ void ln(float4 (&g)[2], float4 (&e)[2]) const {
        g[0] = wbv4(wb, Phase<P>::LN, kq); g[1] = wbv4(wb, Phase<P>::LN + 16, kq);
        e[0] = wbv4(wb, Phase<P>::LN + 32, kq); e[1] = wbv4(wb, Phase<P>::LN + 48, kq);
    }
    template <int P>
    __device__ __forceinline__ void begin(const mpl_block_weights&, const mpl_block_weights&, bool) {}
};

// One Linear phase: mt x NT output tiles, dealt to the 8 waves as contiguous ranges [lo, hi) of the row-major tile list.  A wave
// forms the A fragments of a row tile once (a_frags) and tests each column tile against its range -- static column indices keep the
// fragment form's weights in registers.  THE tile body of both forms: A -> tile_k32 per 32 of k -> epilogue(m, n, accumulator, bias).
template <int P, class Weights, class AFrags, class Epilogue>
__device__ __forceinline__ void linear_phase(const Weights& W, int mt, int wave, bool skip, AFrags a_frags, Epilogue epilogue) {
    constexpr int NT = Phase<P>::NT, KH = Phase<P>::KH;
    const int lo = (mt * NT * wave) / NWAVE, hi = (mt * NT * (wave + 1)) / NWAVE;
    for (int m = lo / NT; m * NT < hi && !skip; ++m) {
        float4 a[KH];
        a_frags(m, a);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int u = m * NT + n;
            if (u < lo || u >= hi) continue;
            float4 w[KH];
            float bias;
            W.template tile<P>(n, w, bias);
            f32x4 c = tile_k32(a[0], a[1], w[0], w[1]);
            if constexpr (KH == 4) c = c + tile_k32(a[2], a[3], w[2], w[3]);
            epilogue(m, n, c, bias);
        }
    }
}

template <bool STAGED>
__global__ __launch_bounds__(NTHR, 1) void spt_kernel(const SptParams p) {
    extern __shared__ __attribute__((aligned(1024))) float smem[];
    constexpr int RX = STAGED ? SPT_SMALL_ROWS : ROWS;
    float* WB = smem;                                   // STAGED: two staged blocks in front (1-KiB aligned pieces)
    float* X = smem + (STAGED ? 2 * SPT_WB_FLOATS : 0);
    float* Q = X + RX * XS;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kq = lane >> 4;
    const int view = blockIdx.x % p.V;
    const int b0 = (blockIdx.x / p.V) * p.spw;
    const mpl_spt_set set = p.sets[(p.flags & MPL_F_MULTI_SPT) ? view : 0];
    const float *pose = p.poses[view], *ray = p.rays[view], *cen = p.centers[view];
    // Few sequences (B V below the 16 x CU count a full launch needs) are SPREAD: p.spw = 1 .. 16 sequences per workgroup, rows
    // sequence-major, so the live rows are the first 17 nl and only their `mt` row tiles are walked (a single frame: one sequence
    // = 2 row tiles per workgroup instead of 17 mostly empty ones).  The arithmetic of a row does not depend on spw.
    const int nl = p.B - b0 < p.spw ? p.B - b0 : p.spw;
    const int rows_live = nl * SJ;
    const int mt = (rows_live + 15) >> 4;

    // weights of the first Block application: issue the loads before anything else
    std::conditional_t<STAGED, StagedWeights, FragWeights> W;
    W.li = li, W.kq = kq;
    if constexpr (STAGED) W.lane = lane;
    mpl_block_weights bw, bw_next;
    if (p.n_apps > 0) {
        bw = set.blocks[p.sched[0] & 0x7f];
        if constexpr (STAGED) stage_block(bw, WB, wave, lane, 0, NWAVE);
        else W.template load<P_QKV>(bw);
        // STAGED: the pointers of an application are fetched one application ahead of the requests that need them
        if (STAGED && p.n_apps > 1) bw_next = set.blocks[p.sched[1] & 0x7f];
    }

    // ---------------- phase 0: joint embedding (:355-396) ----------------
    spt_embed<false>(p, set, X, tid, b0, pose, ray, cen, nl, mt * 16);
    // STAGED: nothing inside the application loop may come by a vector load from global memory -- the compiler's vmcnt(0) in front
    // of its use would wait for the block in flight.  The schedule bytes and the confidences of the live rows (the weighted
    // applications, :61-62) therefore wait in the free tails of the two vector regions.
    unsigned char* sched_l = reinterpret_cast<unsigned char*>(WB + SPT_WB_FLOATS + SPT_WB_VEC + 352);      // [MPL_MAX_APPS]
    float* conf_l = WB + SPT_WB_VEC + 352;                                                                  // [SPT_SMALL_ROWS]
    if (STAGED) {
        if (tid < MPL_MAX_APPS) sched_l[tid] = p.sched[tid];
        for (int r = tid; r < rows_live; r += NTHR) {
            const int sq = r / SJ;
            conf_l[r] = pose[((size_t)(b0 + sq) * SJ + (r - sq * SJ)) * 3 + 2];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of the first block have landed
    }
    __syncthreads();

    // ---------------- block applications (:405-410) ----------------
    const int abl = spt_abl(p);
    const bool no_mfma = (abl & 4) != 0;
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, tlast = (abl & 16) ? __builtin_amdgcn_s_memtime() : 0;
    auto stamp = [&](int k) {
        if (abl & 16) { const unsigned long long now = __builtin_amdgcn_s_memtime(); ph[k] += now - tlast; tlast = now; }
    };
    // A fragments of row tile m: LayerNorm'ed X (qkv, fc1) or Q as it stands (proj: K = 32, fc2: K = 64)
    float4 g[2], e[2];
    auto a_ln = [&](int m, float4 (&a)[2]) { ln_frags(X, m, li, kq, g[0], g[1], e[0], e[1], a[0], a[1]); };
    auto a_q = [&](int m, auto& a) {
        const float* ar = Q + (m * 16 + li) * QS + 4 * kq;
#pragma unroll
        for (int q = 0; q < (int)(sizeof(a) / sizeof(a[0])); ++q) a[q] = ld4(ar + 16 * q);
    };
    // epilogue of proj and fc2: the residual stream takes the tile
    auto add_to_x = [&](int m, int n, const f32x4& c, float b) {
        float* xd = X + (m * 16 + 4 * kq) * XS + n * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) xd[r * XS] += c[r] + b;
    };
    for (int app = 0; app < p.n_apps; ++app) {
        const bool weighted = ((STAGED ? sched_l[app] : p.sched[app]) & 0x80) != 0;
        const bool more = app + 1 < p.n_apps;
        if (!STAGED && more) bw_next = set.blocks[p.sched[app + 1] & 0x7f];   // pointers only; used two phases later
        if constexpr (STAGED) W.wb = WB + (app & 1) * SPT_WB_FLOATS;
        mpl_block_weights bw_after;

        // ---- QKV = LN1(X) . Wqkv^T + b : 17 x 6 tiles -> Q[:, 0:96]
        W.template begin<P_QKV>(bw, bw_next, more);
        W.template ln<P_QKV>(g, e);
        linear_phase<P_QKV>(W, mt, wave, no_mfma, a_ln, [&](int m, int n, const f32x4& c, float b) {
            float* qd = Q + (m * 16 + 4 * kq) * QS + n * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) qd[r * QS] = c[r] + b;
        });
        __syncthreads();
        stamp(0);

        // STAGED: the block of the next application is requested NOW, by the waves the attention leaves idle (stage_block).  Its readers
        // finished an application ago.
        if (STAGED && more) {
            const int busy = (rows_live * SH + 63) >> 6;                  // waves with attention work
            const int w0 = busy < NWAVE - 1 ? busy : 0;
            stage_block(bw_next, WB + ((app + 1) & 1) * SPT_WB_FLOATS, wave, lane, w0, NWAVE - w0);
            if (app + 2 < p.n_apps) bw_after = set.blocks[sched_l[app + 2] & 0x7f];
        }
        stamp(5);
        // ---- attention: thread per (row, head); 17 scores in registers (:55-64)
        for (int pr = tid; pr < rows_live * SH && !(abl & 1); pr += NTHR) {
            const int r = pr >> 3, h = pr & 7;
            const int sq = r / SJ;
            const float* kb = Q + (sq * SJ) * QS + SD + 4 * h;
            const float4 q = ld4(Q + r * QS + 4 * h);
            float sc[SJ];
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                const float4 k = ld4(kb + j * QS);
                sc[j] = 0.5f * (fmaf(q.x, k.x, q.y * k.y) + fmaf(q.z, k.z, q.w * k.w));  // hd^-0.5 = 0.5
                mx = fmaxf(mx, sc[j]);
            }
            float l = 0.f;
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                sc[j] = __expf(sc[j] - mx);
                l += sc[j];
            }
            float inv = 1.0f / l;
            if (weighted) {  // attn * conf_weights.unsqueeze(1) after softmax (:61-62): scales query row r
                const int b = b0 + sq;
                if (STAGED) inv *= conf_l[r];
                else inv *= (b < p.B) ? pose[((size_t)b * SJ + (r - sq * SJ)) * 3 + 2] : 0.f;
            }
            float4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < SJ; ++j) {
                const float4 v = ld4(kb + j * QS + SD);
                const float pj = sc[j] * inv;
                o.x = fmaf(pj, v.x, o.x);
                o.y = fmaf(pj, v.y, o.y);
                o.z = fmaf(pj, v.z, o.z);
                o.w = fmaf(pj, v.w, o.w);
            }
            st4(Q + r * QS + 4 * h, o);  // overwrite q (only this thread ever reads it)
        }
        __syncthreads();
        stamp(1);

        // ---- X += attn_out . Wproj^T + b : 17 x 2 tiles
        W.template begin<P_PROJ>(bw, bw_next, more);
        linear_phase<P_PROJ>(W, mt, wave, no_mfma, a_q, add_to_x);
        __syncthreads();
        stamp(2);

        // ---- Hid = gelu(LN2(X) . W1^T + b) : 17 x 4 tiles -> Q[:, 0:64]
        W.template begin<P_FC1>(bw, bw_next, more);
        W.template ln<P_FC1>(g, e);
        linear_phase<P_FC1>(W, mt, wave, no_mfma, a_ln, [&](int m, int n, const f32x4& c, float b) {
            float* qd = Q + (m * 16 + 4 * kq) * QS + n * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) qd[r * QS] = (abl & 2) ? (c[r] + b) : gelu_erf(c[r] + b);
        });
        __syncthreads();
        stamp(3);

        // ---- X += Hid . W2^T + b : K = 64, 17 x 2 tiles
        W.template begin<P_FC2>(bw, bw_next, more);
        linear_phase<P_FC2>(W, mt, wave, no_mfma, a_q, add_to_x);
        if (STAGED) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of the next block have landed
        __syncthreads();
        stamp(4);
        bw = bw_next;
        if (STAGED && app + 2 < p.n_apps) bw_next = bw_after;
    }

    if (abl & 16) {                             // laboratory builds: cycle counts per phase instead of the stage's output
        if (lane == 0 && blockIdx.x < 32) {
            float* o = p.xs + (size_t)(blockIdx.x * NWAVE + wave) * 8;
            for (int k = 0; k < 6; ++k) o[k] = (float)ph[k];
        }
        return;
    }
    spt_epilogue<false>(p, X, tid, view, b0, pose, ray, cen, nl, rows_live);
}

int launch_spt_native(const SptParams& p, int form, int grid, hipStream_t s) {
    // >64 KiB of dynamic LDS needs an explicit opt-in, once per device
    if (form == MPL_SPT_STAGED) {
        if (int rc = kernel_lds_once<spt_kernel<true>>(SPT_SMALL_LDS_BYTES)) return rc;
        hipLaunchKernelGGL(spt_kernel<true>, dim3(grid), dim3(NTHR), SPT_SMALL_LDS_BYTES, s, p);
    } else {
        if (int rc = kernel_lds_once<spt_kernel<false>>(SPT_LDS_BYTES)) return rc;
        hipLaunchKernelGGL(spt_kernel<false>, dim3(grid), dim3(NTHR), SPT_LDS_BYTES, s, p);
    }
    return hip_check_launch();
}

}  // namespace mpl
