// The fused spatial stage (mpl_spt_tokens): joint embedding + the whole SPT block stack + Spatial_norm + per-view glue in one
// launch, the token matrix resident in LDS for all L + 1 block applications.  This header is what the stage's kernels share:
// geometry, the launch parameters, the embedding in front of the block applications and the epilogue behind them.
//
// Reference (MPL/lib/models/multiview_mpl.py): Spatial_forward_features :349-414 (embedding :355-385, optional 3D position
// encoding :389-396, block loop with the last block applied twice :405-410, Spatial_norm :412) and the per-view part of forward
// :458-492 (confidence_in_FPT :465-467, ray embedding concat :469-471 / :486-489, 3D position embedding :474-483, flatten :491).
//
// Geometry: J = 17 joints, d = 32, H = 8 heads of dim 4, MLP hidden 64.  A workgroup is 512 threads = 8 waves, two per SIMD, one
// workgroup per CU (147968 B of LDS or more); it owns up to SEQ = 16 sequences of one view = up to 272 token rows = 17 MFMA
// row tiles of 16.  Who runs what (spt.hip: spt_form, launch_spt): precision "fp32" (every block carries the packed operand of
// mpl_spt_pack) -> spt_packed.hip spt3_kernel<SS>;  "fp32_mfma" / nn.Linear weights only -> spt_native.hip spt_kernel<true> (staged,
// up to 8 sequences per workgroup) or <false> (fragments, 9 .. 16);  every shape but 17 / 32 / 8, and MPL_F_GENERIC_SPT -> spt_any.hip.
#pragma once
#include "common.hpp"

namespace mpl {

constexpr int SJ = 17;          // joints
constexpr int SD = 32;          // embed_dim_ratio
constexpr int SH = 8;           // heads
constexpr int SEQ = 16;         // sequences per workgroup, at most
constexpr int ROWS = SEQ * SJ;  // 272
constexpr int XS = 36;          // X row stride (floats)
constexpr int NTHR = 512;       // 8 waves: two per SIMD
constexpr int NWAVE = NTHR / 64;
constexpr int SPT_SMALL_SPW = 8;    // up to this many sequences per workgroup the native kernel runs its staged form (spt_form)

struct SptParams {
    const float* poses[MPL_MAX_VIEWS];
    const float* rays[MPL_MAX_VIEWS];
    const float* centers[MPL_MAX_VIEWS];
    const mpl_spt_set* sets;
    const float *snorm_w, *snorm_b;
    const float *pos3d_embed, *pos3d_view, *pos3d_lin_w, *pos3d_lin_b;
    const float *ray_w, *ray_b, *cfpt_w, *cfpt_b;
    float* xs;
    int B, V, in_ch, n_apps;
    unsigned flags;
    int c3;  // channel count of the pos_3d_* tensors (d or 2d)
    int spw;  // sequences per workgroup (spt_kernel: 1..16, few sequences spread over the chip; spt3_kernel<SS>: SS)
    int abl;  // MPL_SPT_ABL, laboratory builds only.  spt_kernel: 1 no attention, 2 no GELU, 4 no MFMA phases, 16 cycle counts for the output; spt3_kernel: tools/spt_abl.py
    unsigned* err_host;  // sticky error word of the device (common.hpp device_error_word): bit 1 (value 2) = an operand left its fp16 window
    unsigned char sched[MPL_MAX_APPS];  // layer | weighted << 7
};

// One host function per kernel file: LDS opt-in + launch on `grid` workgroups.  form: MPL_SPT_STAGED / MPL_SPT_FRAGS; ss: 1, 2, 4, 8 or 16
int launch_spt_native(const SptParams& p, int form, int grid, hipStream_t s);
int launch_spt_packed(const SptParams& p, int ss, int grid, hipStream_t s);

// Pointers fetched from device tables carry no address-space information; tell the compiler they are
// global so it emits global_load (vmcnt only) instead of flat_load.
typedef const __attribute__((address_space(1))) float* gfp;
__device__ __forceinline__ gfp G(const float* p) { return (gfp)p; }
__device__ __forceinline__ float4 ld4(gfp p) {
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 t = *reinterpret_cast<const __attribute__((address_space(1))) v4*>(p);
    return make_float4(t.x, t.y, t.z, t.w);
}

// Row order of the token matrix X in LDS.  TM = false: row = sequence * 17 + joint (the fp32-MFMA kernel); TM = true:
// row = joint * 16 + sequence -- token-major: MFMA row tile j holds joint j of the 16 sequences, so a lane of a transposed
// accumulator tile is one (sequence, head) and the attention needs no cross-lane traffic (spt3_kernel).
template <bool TM, int SS = SEQ>
__device__ __forceinline__ void row_to_sj(int r, int& sq, int& j) {
    if (TM) { j = r / SS; sq = r % SS; }       // SS sequences per joint (a power of two): rows beyond 17 SS belong to no joint (j >= 17)
    else { sq = r / SJ; j = r - sq * SJ; }
}

// joint embedding (:355-396) of the workgroup's 16 sequences -> X
template <bool TM, int SS = SEQ>
__device__ __forceinline__ void spt_embed(const SptParams& p, const mpl_spt_set& set, float* X, int tid, int b0,
                                          const float* pose, const float* ray, const float* cen, int nseq = SEQ, int nrows = ROWS) {
    for (int idx = tid; idx < nrows * SD; idx += NTHR) {
        const int r = idx >> 5, c = idx & 31;
        int sq, j;
        row_to_sj<TM, SS>(r, sq, j);
        const int b = b0 + sq;
        float x = 0.f;
        if (b < p.B && sq < nseq && j < SJ) {
            const float* in = pose + ((size_t)b * SJ + j) * 3;
            const float* we = set.embed_w + c * p.in_ch;
            x = set.embed_b[c] + we[0] * in[0] + we[1] * in[1];
            if (p.in_ch == 3) x += we[2] * in[2];
            if (p.flags & MPL_F_CONF_ADD) x += set.conf_w[c] * in[2] + set.conf_b[c];
            if (p.flags & MPL_F_CONF_MULT) x *= set.conf_w[c] * in[2] + set.conf_b[c];
            x += set.pos_embed[j * SD + c];
            if (p.flags & MPL_F_POS3D_SPATIAL) {
                if (p.flags & MPL_F_POS3D_LEARN) {
                    x += p.pos3d_embed[j * p.c3 + c];
                } else {
                    const float* rr = ray + ((size_t)b * SJ + j) * 3;
                    const float* cc = cen + (size_t)b * 3;
                    const float vx = rr[0] - cc[0], vy = rr[1] - cc[1], vz = rr[2] - cc[2];
                    const float nrm = fmaxf(sqrtf(vx * vx + vy * vy + vz * vz), 1e-12f);  // F.normalize eps
                    const float* wl = p.pos3d_lin_w + c * 3;
                    x += p.pos3d_lin_b[c] + wl[0] * (vx / nrm) + wl[1] * (vy / nrm) + wl[2] * (vz / nrm);
                }
            }
        }
        X[r * XS + c] = x;
    }
}

// Spatial_norm (:412) + per-view glue (:465-491) -> xs[b*V+v][...]
template <bool TM, int SS = SEQ>
__device__ __forceinline__ void spt_epilogue(const SptParams& p, const float* X, int tid, int view, int b0, const float* pose,
                                             const float* ray, const float* cen, int nseq = SEQ, int nrows = ROWS) {
    const bool to_rays = (p.flags & MPL_F_POS3D_TO_RAYS) && (p.flags & MPL_F_RAYS_TOKEN);   // feature concat (:469-471)
    const bool ray_tok = !(p.flags & MPL_F_POS3D_TO_RAYS) && (p.flags & MPL_F_RAYS_TOKEN);  // token concat (:486-489)
    const int cw = to_rays ? 2 * SD : SD;                 // channels per joint in the output row
    const int Df = SJ * SD * ((p.flags & MPL_F_RAYS_TOKEN) ? 2 : 1);
    for (int r = tid; r < nrows; r += NTHR) {
        int sq, j;
        row_to_sj<TM, SS>(r, sq, j);
        const int b = b0 + sq;
        if (b >= p.B || sq >= nseq || j >= SJ) continue;
        const float* xr = X + r * XS;
        float v[SD];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < SD; c += 4) {
            const float4 t = ld4(xr + c);
            v[c] = t.x; v[c + 1] = t.y; v[c + 2] = t.z; v[c + 3] = t.w;
            s += (t.x + t.y) + (t.z + t.w);
        }
        const float mean = s * (1.0f / 32.0f);
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < SD; ++c) {
            v[c] -= mean;
            ss = fmaf(v[c], v[c], ss);
        }
        const float rstd = 1.0f / sqrtf(ss * (1.0f / 32.0f) + 1e-6f);
        const float conf = pose[((size_t)b * SJ + j) * 3 + 2];
        float dx = 0.f, dy = 0.f, dz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        const bool need_dir = (p.flags & MPL_F_RAYS_TOKEN) ||
                              (!(p.flags & MPL_F_POS3D_SPATIAL) && !(p.flags & MPL_F_POS3D_LEARN));
        if (need_dir) {
            const float* rr = ray + ((size_t)b * SJ + j) * 3;
            const float* cc = cen + (size_t)b * 3;
            dx = rr[0] - cc[0]; dy = rr[1] - cc[1]; dz = rr[2] - cc[2];
            const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
            nx = dx / nrm; ny = dy / nrm; nz = dz / nrm;
        }
        // 3D position term for channel c of this joint (:474-483)
        auto pos3d = [=](int c) -> float {
            if (p.flags & MPL_F_POS3D_SPATIAL) return p.pos3d_view[j * p.c3 + c];
            if (p.flags & MPL_F_POS3D_LEARN) return p.pos3d_embed[j * p.c3 + c];
            const float* wl = p.pos3d_lin_w + c * 3;
            return p.pos3d_lin_b[c] + wl[0] * nx + wl[1] * ny + wl[2] * nz;
        };
        auto ray_emb = [=](int c) -> float {
            const float* wr = p.ray_w + c * 3;
            return p.ray_b[c] + wr[0] * dx + wr[1] * dy + wr[2] * dz;
        };
        float* orow = p.xs + ((size_t)b * p.V + view) * Df;
        float* o1 = orow + j * cw;
#pragma unroll
        for (int c = 0; c < SD; c += 4) {
            float t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float y = v[c + q] * rstd * p.snorm_w[c + q] + p.snorm_b[c + q];
                if (p.flags & MPL_F_CONF_IN_FPT) y += p.cfpt_w[c + q] * conf + p.cfpt_b[c + q];
                t[q] = y + pos3d(c + q);
            }
            st4(o1 + c, float4{t[0], t[1], t[2], t[3]});
        }
        if (to_rays) {
#pragma unroll
            for (int c = 0; c < SD; c += 4) {
                float t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = ray_emb(c + q) + pos3d(SD + c + q);
                st4(o1 + SD + c, float4{t[0], t[1], t[2], t[3]});
            }
        } else if (ray_tok) {
            float* o2 = orow + (SJ + j) * SD;
#pragma unroll
            for (int c = 0; c < SD; c += 4) st4(o2 + c, float4{ray_emb(c), ray_emb(c + 1), ray_emb(c + 2), ray_emb(c + 3)});
        }
    }
}

}  // namespace mpl
