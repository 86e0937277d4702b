// Shape-general spatial stage: joint embedding + the SPT block stack + Spatial_norm + per-view glue for ANY number of joints J,
// width d and head count H (run-time values), fp32 throughout.  launch_spt (spt.hip) sends every configuration that is not
// 17 / 32 / 8 here, and also 17 / 32 / 8 when mpl_config.flags carries MPL_F_GENERIC_SPT.
//
// Reference (MPL/lib/models/multiview_mpl.py): Spatial_forward_features :349-414 (embedding :355-385, 3D position encoding
// in the spatial stage :389-396, block loop with the last block applied twice and, with
// confidence_as_attention_uncertainty_weight, every block first applied once with row weights :405-410, Spatial_norm :412),
// Block :84-92, Attention :53-67, Mlp :31-37, and the per-view part of forward :458-492 (confidence_in_FPT :465-467, ray
// embedding concat :469-471 / :486-489, 3D position embedding :474-483, flatten :491).
//
// Geometry: one 256-thread workgroup owns S sequences of one view (S * J token rows).  Its token rows stay in LDS for the whole
// stack: X (residual stream), A (LayerNorm output, then the attention output), T (q | k | v, then the MLP hidden layer), all with
// odd row strides.  The Linear layers read the nn.Linear tensors in place, streamed through a 64 x 32 LDS tile (12 d^2 floats per
// block are never held whole).  Arithmetic: LayerNorm eps 1e-6 with two-pass variance, exact-erf GELU, scores (q.k) * hd^-0.5
// scaled after the product, softmax with max subtraction, plain fmaf products in a fixed k order: every row's result is
// independent of S and of the batch.
#include "common.hpp"

namespace mpl {

namespace {

constexpr int SA_THR = 256;
constexpr int SA_NT = 64;                 // output columns per GEMM tile
constexpr int SA_MT = 64;                 // output rows per GEMM tile (16 row groups x 4)
constexpr int SA_KC = 32;                 // k chunk of a staged weight tile
constexpr int SA_WS = SA_KC + 1;          // row stride of the staged weight tile
constexpr int SA_W_FLOATS = SA_NT * SA_WS;

struct SptAnyParams {
    const float* poses[MPL_MAX_VIEWS];
    const float* rays[MPL_MAX_VIEWS];
    const float* centers[MPL_MAX_VIEWS];
    const mpl_spt_set* sets;
    const float *snorm_w, *snorm_b;
    const float *pos3d_embed, *pos3d_view, *pos3d_lin_w, *pos3d_lin_b;
    const float *ray_w, *ray_b, *cfpt_w, *cfpt_b;
    float* xs;
    int B, V, J, d, H, in_ch, n_apps, spw;
    int xs_ld, ts_ld;                     // LDS row strides of X / A and of T (floats)
    unsigned flags;
    int c3;                               // channel count of the pos_3d_* tensors (d or 2d)
    float scale;                          // hd^-0.5
    unsigned char sched[MPL_MAX_APPS];    // layer | weighted << 7
};

inline int odd_stride(int n) { return n | 1; }

// O[r][n] (=, gelu =, +=) sum_k A[r][k] W[n][k] + bias[n] for r < R, n < N.  W is an nn.Linear weight [N][K] in global memory.
// Thread (tr, tc) of a 64 x 64 output tile owns rows tr + 16 q and columns tc + 16 u (q, u < 4): LDS reads of A are broadcasts
// within a 16-lane group, reads of the staged weight tile hit 16 distinct banks.
template <int EPI>
__device__ void sa_gemm(const float* A, int lda, int R, int K, const float* __restrict__ W, const float* __restrict__ bias, int N,
                        float* O, int ldo, float* Wt) {
    const int tid = threadIdx.x, tc = tid & 15, tr = tid >> 4;
    for (int n0 = 0; n0 < N; n0 += SA_NT) {
        for (int r0 = 0; r0 < R; r0 += SA_MT) {
            float acc[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[q][u] = 0.f;
            const float* ar[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + tr + 16 * q;
                ar[q] = A + (size_t)(r < R ? r : 0) * lda;
            }
            for (int k0 = 0; k0 < K; k0 += SA_KC) {
                const int kc = K - k0 < SA_KC ? K - k0 : SA_KC;
                __syncthreads();                                   // the previous tile's readers are done
                for (int i = tid; i < SA_NT * SA_KC; i += SA_THR) {
                    const int n = i / SA_KC, k = i - n * SA_KC;
                    Wt[n * SA_WS + k] = (n0 + n < N && k < kc) ? W[(size_t)(n0 + n) * K + k0 + k] : 0.f;
                }
                __syncthreads();
                for (int k = 0; k < kc; ++k) {
                    float a[4], w[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[q] = ar[q][k0 + k];
#pragma unroll
                    for (int u = 0; u < 4; ++u) w[u] = Wt[(tc + 16 * u) * SA_WS + k];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[q][u] = fmaf(a[q], w[u], acc[q][u]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + tr + 16 * q;
                if (r >= R) continue;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int n = n0 + tc + 16 * u;
                    if (n >= N) continue;
                    const float v = acc[q][u] + bias[n];
                    float* o = O + (size_t)r * ldo + n;
                    if (EPI == MPL_EPI_BIAS_RESIDUAL) *o += v;
                    else if (EPI == MPL_EPI_BIAS_GELU) *o = gelu_erf(v);
                    else *o = v;
                }
            }
        }
    }
    __syncthreads();
}

// Y[r] = LayerNorm(X[r]) over d channels (eps 1e-6, two-pass), one wave per row
__device__ void sa_layernorm(const float* X, float* Y, int R, int d, int ld, const float* __restrict__ g, const float* __restrict__ b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < R; r += SA_THR / 64) {
        const float* xr = X + (size_t)r * ld;
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += xr[c];
        const float mean = wave_sum(s) / (float)d;
        float ss = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float t = xr[c] - mean;
            ss += t * t;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)d + 1e-6f);
        for (int c = lane; c < d; c += 64) Y[(size_t)r * ld + c] = (xr[c] - mean) * rstd * g[c] + b[c];
    }
    __syncthreads();
}

// Attention :55-64 on T = [q | k | v] (row stride ts): one thread per (token row, head); the scores are recomputed per pass (max,
// sum, P.V) instead of being held, the output accumulates in place in O.  rw != nullptr: the softmax rows are multiplied by the
// confidence of their query token (:61-62).
__device__ void sa_attention(const SptAnyParams& p, const float* T, float* O, int R, const float* pose, int b0) {
    const int J = p.J, d = p.d, H = p.H, hd = d / H, ts = p.ts_ld, xs = p.xs_ld;
    for (int t = threadIdx.x; t < R * H; t += SA_THR) {
        const int r = t / H, h = t - r * H;
        const int sq = r / J;
        const float* q = T + (size_t)r * ts + h * hd;
        const float* kb = T + (size_t)sq * J * ts + d + h * hd;
        auto score = [&](int j) {
            const float* k = kb + (size_t)j * ts;
            float s = 0.f;
            for (int e = 0; e < hd; ++e) s = fmaf(q[e], k[e], s);
            return s * p.scale;
        };
        float mx = -INFINITY;
        for (int j = 0; j < J; ++j) mx = fmaxf(mx, score(j));
        float l = 0.f;
        for (int j = 0; j < J; ++j) l += __expf(score(j) - mx);
        float inv = 1.0f / l;
        float* o = O + (size_t)r * xs + h * hd;
        for (int e = 0; e < hd; ++e) o[e] = 0.f;
        for (int j = 0; j < J; ++j) {
            const float pj = __expf(score(j) - mx) * inv;
            const float* v = kb + (size_t)j * ts + d;
            for (int e = 0; e < hd; ++e) o[e] = fmaf(pj, v[e], o[e]);
        }
        if (pose) {
            const int b = b0 + sq, j = r - sq * J;
            const float w = pose[((size_t)b * J + j) * 3 + 2];
            for (int e = 0; e < hd; ++e) o[e] *= w;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(SA_THR) void spt_any_kernel(const SptAnyParams p) {
    extern __shared__ __attribute__((aligned(16))) float sa_smem[];
    const int J = p.J, d = p.d, xs = p.xs_ld, ts = p.ts_ld;
    const int view = blockIdx.x % p.V, b0 = (blockIdx.x / p.V) * p.spw;
    const int nseq = p.B - b0 < p.spw ? p.B - b0 : p.spw;
    const int R = nseq * J;
    float* X = sa_smem;
    float* A = X + (size_t)p.spw * J * xs;
    float* T = A + (size_t)p.spw * J * xs;
    float* Wt = T + (size_t)p.spw * J * ts;
    const mpl_spt_set set = p.sets[(p.flags & MPL_F_MULTI_SPT) ? view : 0];
    const float* pose = p.poses[view];
    const float* ray = p.rays[view];
    const float* cen = p.centers[view];
    const int tid = threadIdx.x;

    // ---- joint embedding (:355-396) -> X
    for (int idx = tid; idx < R * d; idx += SA_THR) {
        const int r = idx / d, c = idx - r * d;
        const int sq = r / J, j = r - sq * J, b = b0 + sq;
        const float* in = pose + ((size_t)b * J + j) * 3;
        const float* we = set.embed_w + c * p.in_ch;
        float x = set.embed_b[c] + we[0] * in[0] + we[1] * in[1];
        if (p.in_ch == 3) x += we[2] * in[2];
        if (p.flags & MPL_F_CONF_ADD) x += set.conf_w[c] * in[2] + set.conf_b[c];
        if (p.flags & MPL_F_CONF_MULT) x *= set.conf_w[c] * in[2] + set.conf_b[c];
        x += set.pos_embed[j * d + c];
        if (p.flags & MPL_F_POS3D_SPATIAL) {
            if (p.flags & MPL_F_POS3D_LEARN) {
                x += p.pos3d_embed[j * p.c3 + c];
            } else {
                const float* rr = ray + ((size_t)b * J + j) * 3;
                const float* cc = cen + (size_t)b * 3;
                const float vx = rr[0] - cc[0], vy = rr[1] - cc[1], vz = rr[2] - cc[2];
                const float nrm = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);  // F.normalize eps
                const float* wl = p.pos3d_lin_w + c * 3;
                x += p.pos3d_lin_b[c] + wl[0] * (vx / nrm) + wl[1] * (vy / nrm) + wl[2] * (vz / nrm);
            }
        }
        X[(size_t)r * xs + c] = x;
    }
    __syncthreads();

    // ---- the block stack (:405-410)
    for (int a = 0; a < p.n_apps; ++a) {
        const mpl_block_weights bw = set.blocks[p.sched[a] & 0x7f];
        const bool weighted = (p.sched[a] & 0x80) != 0;
        // x = x + proj(attn(qkv(norm1(x))))
        sa_layernorm(X, A, R, d, xs, bw.ln1_w, bw.ln1_b);
        sa_gemm<MPL_EPI_BIAS>(A, xs, R, d, bw.qkv_w, bw.qkv_b, 3 * d, T, ts, Wt);
        sa_attention(p, T, A, R, weighted ? pose : nullptr, b0);
        sa_gemm<MPL_EPI_BIAS_RESIDUAL>(A, xs, R, d, bw.proj_w, bw.proj_b, d, X, xs, Wt);
        // x = x + fc2(gelu(fc1(norm2(x))))
        sa_layernorm(X, A, R, d, xs, bw.ln2_w, bw.ln2_b);
        sa_gemm<MPL_EPI_BIAS_GELU>(A, xs, R, d, bw.fc1_w, bw.fc1_b, 2 * d, T, ts, Wt);
        sa_gemm<MPL_EPI_BIAS_RESIDUAL>(T, ts, R, 2 * d, bw.fc2_w, bw.fc2_b, d, X, xs, Wt);
    }

    // ---- Spatial_norm (:412) + per-view glue (:465-491) -> xs[b*V+v][...], one wave per token row
    const bool to_rays = (p.flags & MPL_F_POS3D_TO_RAYS) && (p.flags & MPL_F_RAYS_TOKEN);   // feature concat (:469-471)
    const bool ray_tok = !(p.flags & MPL_F_POS3D_TO_RAYS) && (p.flags & MPL_F_RAYS_TOKEN);  // token concat (:486-489)
    const bool need_dir = (p.flags & MPL_F_RAYS_TOKEN) || (!(p.flags & MPL_F_POS3D_SPATIAL) && !(p.flags & MPL_F_POS3D_LEARN));
    const int cw = to_rays ? 2 * d : d;                   // channels per joint in the output row
    const int Df = J * d * ((p.flags & MPL_F_RAYS_TOKEN) ? 2 : 1);
    const int lane = tid & 63;
    for (int r = tid >> 6; r < R; r += SA_THR / 64) {
        const int sq = r / J, j = r - sq * J, b = b0 + sq;
        const float* xr = X + (size_t)r * xs;
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += xr[c];
        const float mean = wave_sum(s) / (float)d;
        float ss = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float t = xr[c] - mean;
            ss += t * t;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)d + 1e-6f);
        const float conf = pose[((size_t)b * J + j) * 3 + 2];
        float dx = 0.f, dy = 0.f, dz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        if (need_dir) {
            const float* rr = ray + ((size_t)b * J + j) * 3;
            const float* cc = cen + (size_t)b * 3;
            dx = rr[0] - cc[0]; dy = rr[1] - cc[1]; dz = rr[2] - cc[2];
            const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
            nx = dx / nrm; ny = dy / nrm; nz = dz / nrm;
        }
        auto pos3d = [&](int c) -> float {            // 3D position term of channel c of this joint (:474-483)
            if (p.flags & MPL_F_POS3D_SPATIAL) return p.pos3d_view[j * p.c3 + c];
            if (p.flags & MPL_F_POS3D_LEARN) return p.pos3d_embed[j * p.c3 + c];
            const float* wl = p.pos3d_lin_w + c * 3;
            return p.pos3d_lin_b[c] + wl[0] * nx + wl[1] * ny + wl[2] * nz;
        };
        auto ray_emb = [&](int c) -> float {
            const float* wr = p.ray_w + c * 3;
            return p.ray_b[c] + wr[0] * dx + wr[1] * dy + wr[2] * dz;
        };
        float* orow = p.xs + ((size_t)b * p.V + view) * Df;
        float* o1 = orow + (size_t)j * cw;
        for (int c = lane; c < d; c += 64) {
            float y = (xr[c] - mean) * rstd * p.snorm_w[c] + p.snorm_b[c];
            if (p.flags & MPL_F_CONF_IN_FPT) y += p.cfpt_w[c] * conf + p.cfpt_b[c];
            o1[c] = y + pos3d(c);
            if (to_rays) o1[d + c] = ray_emb(c) + pos3d(d + c);
            else if (ray_tok) orow[(size_t)(J + j) * d + c] = ray_emb(c);
        }
    }
}

}  // namespace

// LDS bytes of one token row (X, A and T with their odd strides) and the most sequences a workgroup holds within 64 KiB (two
// or more workgroups per CU), at least one
size_t spt_any_row_bytes(int d) { return (size_t)(2 * odd_stride(d) + odd_stride(3 * d)) * sizeof(float); }
int spt_any_seq_cap(int J, int d) {
    const int s_lds = (int)((64 * 1024 - SA_W_FLOATS * sizeof(float)) / (spt_any_row_bytes(d) * J));
    return s_lds < 1 ? 1 : s_lds;
}

int launch_spt_any(const mpl_config* cfg, const mpl_weights* w, const mpl_inputs* in, float* xs, hipStream_t s) {
    if (mpl_config_supported(cfg) != MPL_OK) return MPL_E_UNSUPPORTED;
    if (!w || !in || !xs || in->batch <= 0 || !w->spt_sets || !w->spatial_norm_w || !w->spatial_norm_b) return MPL_E_INVALID;
    if (cfg->in_chans != 2 && cfg->in_chans != 3) return MPL_E_INVALID;
    const unsigned f = cfg->flags;
    const int J = cfg->num_joints, d = cfg->dim, V = cfg->num_views, B = in->batch;
    SptAnyParams p;
    const bool needs_rays = (f & MPL_F_RAYS_TOKEN) || !(f & MPL_F_POS3D_LEARN);
    for (int v = 0; v < MPL_MAX_VIEWS; ++v) {
        const bool on = v < V;
        p.poses[v] = on ? in->poses[v] : nullptr;
        p.rays[v] = on ? in->rays[v] : nullptr;
        p.centers[v] = on ? in->centers[v] : nullptr;
        if (on && !p.poses[v]) return MPL_E_INVALID;
        if (on && needs_rays && (!p.rays[v] || !p.centers[v])) return MPL_E_INVALID;
    }
    p.sets = w->spt_sets;
    p.snorm_w = w->spatial_norm_w; p.snorm_b = w->spatial_norm_b;
    p.pos3d_embed = w->pos_3d_embed; p.pos3d_view = w->pos_3d_view_coding;
    p.pos3d_lin_w = w->pos_3d_linear_w; p.pos3d_lin_b = w->pos_3d_linear_b;
    p.ray_w = w->ray_embed_w; p.ray_b = w->ray_embed_b;
    p.cfpt_w = w->conf_fpt_w; p.cfpt_b = w->conf_fpt_b;
    if ((f & MPL_F_RAYS_TOKEN) && (!p.ray_w || !p.ray_b)) return MPL_E_INVALID;
    if ((f & MPL_F_CONF_IN_FPT) && (!p.cfpt_w || !p.cfpt_b)) return MPL_E_INVALID;
    p.xs = xs;
    p.B = B; p.V = V; p.J = J; p.d = d; p.H = cfg->heads; p.in_ch = cfg->in_chans;
    p.flags = f;
    p.c3 = (f & MPL_F_POS3D_TO_RAYS) ? 2 * d : d;
    p.scale = 1.0f / sqrtf((float)(d / cfg->heads));
    p.xs_ld = odd_stride(d);
    p.ts_ld = odd_stride(3 * d);
    // schedule (:405-410): [blk(x,w)]; if last: blk(x); blk(x)
    int n = 0;
    if (!(f & MPL_F_NO_SPT)) {
        for (int l = 0; l < cfg->depth; ++l) {
            if (n + 3 > MPL_MAX_APPS) return MPL_E_UNSUPPORTED;
            if (f & MPL_F_CONF_ATTN_W) p.sched[n++] = (unsigned char)(l | 0x80);
            if (l == cfg->depth - 1) p.sched[n++] = (unsigned char)l;
            p.sched[n++] = (unsigned char)l;
        }
    }
    p.n_apps = n;
    int cus = 0;
    if (int rc = device_cu_count(&cus)) return rc;
    // Sequences per workgroup: spt_form (spt.hip), the one rule mpl_spt_form reports by; a sequence that alone needs more than
    // 64 KiB gets a workgroup of its own (J d <= 4096: < 84 KiB).
    int spw = 0;
    const int form = spt_form(cfg, B, 0, cus, &spw);
    if (form < 0) return form;
    if (form != MPL_SPT_ANY) return MPL_E_INVALID;       // a configuration launch_spt keeps for the tuned kernels
    p.spw = spw;
    const size_t row_bytes = spt_any_row_bytes(d), w_bytes = SA_W_FLOATS * sizeof(float);
    const size_t lds = (size_t)spw * J * row_bytes + w_bytes;
    if (int rc = kernel_lds_once<spt_any_kernel>(160 * 1024)) return rc;
    if (lds > 160 * 1024) return MPL_E_UNSUPPORTED;
    const long long grid = (long long)V * ((B + spw - 1) / spw);
    if (grid > 0x7fffffffll) return MPL_E_UNSUPPORTED;
    ProfScope prof(MPL_K_SPT, s);
    hipLaunchKernelGGL(spt_any_kernel, dim3((unsigned)grid), dim3(SA_THR), lds, s, p);
    return hip_check_launch();
}

}  // namespace mpl
