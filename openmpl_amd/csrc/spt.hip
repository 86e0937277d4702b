// Host side of the fused spatial stage (spt_stage.hpp): the launch rule, and the launcher that checks the arguments, fills the
// parameters and the block schedule and hands the launch to the kernel file of the chosen form -- spt_packed.hip (packed
// operands), spt_native.hip (nn.Linear weights, staged or fragment form) or spt_any.hip (every other shape).
#include <stdlib.h>

#include "spt_stage.hpp"

namespace mpl {

// every other shape, and 17 / 32 / 8 on request, runs on the shape-general kernel (spt_any.hip)
static bool spt_shape_general(const mpl_config* cfg) {
    return cfg->num_joints != SJ || cfg->dim != SD || cfg->heads != SH || (cfg->flags & MPL_F_GENERIC_SPT);
}

// THE rule by which an SPT launch picks its kernel and its sequences per workgroup: launch_spt and launch_spt_any launch by it,
// mpl_spt_form reports by it.  As few sequences per workgroup as keep the launch inside one wave of workgroups (one per CU), so
// that a single frame or a few hundred sequences use the whole chip with 2-3 live row tiles per workgroup instead of a few
// workgroups with 17: the smallest c with V ceil(B / c) <= cus, at most SEQ for the tuned kernels and spt_any_seq_cap (LDS) for
// the shape-general one.  Tuned, nn.Linear weights: up to SPT_SMALL_SPW per workgroup run the staged form (spt_kernel<true>),
// more the fragment form (spt_native.hip).  Tuned, packed operands: 16, 8, 4, 2 or 1 sequences per workgroup, the next power of two (bitwise the
// same rows; spt3_kernel<SS>, spt_packed.hip).
int spt_form(const mpl_config* cfg, int batch, int use_packed, int cus, int* spw_out) {
    if (!cfg || !spw_out || batch <= 0 || cus < 1 || cfg->num_views < 1 || cfg->num_views > MPL_MAX_VIEWS) return MPL_E_INVALID;
    const bool any = spt_shape_general(cfg);
    if (any && mpl_config_supported(cfg) != MPL_OK) return MPL_E_UNSUPPORTED;
    const int cap = any ? spt_any_seq_cap(cfg->num_joints, cfg->dim) : SEQ;
    int spw = cap;
    for (int c = 1; c < cap; ++c)
        if ((long long)cfg->num_views * ((batch + c - 1) / c) <= cus) { spw = c; break; }
    *spw_out = spw;
    if (any) return MPL_SPT_ANY;
    if (!use_packed) return spw <= SPT_SMALL_SPW ? MPL_SPT_STAGED : MPL_SPT_FRAGS;
    int ss = 1;
    while (ss < spw) ss *= 2;
    *spw_out = ss;
    return MPL_SPT_PACKED;
}

int launch_spt(const mpl_config* cfg, const mpl_weights* w, const mpl_inputs* in, float* xs, int use_packed, hipStream_t s) {
    if (spt_shape_general(cfg)) return launch_spt_any(cfg, w, in, xs, s);
    if (cfg->num_views < 1 || cfg->num_views > MPL_MAX_VIEWS || in->batch <= 0) return MPL_E_INVALID;
    if (cfg->in_chans != 2 && cfg->in_chans != 3) return MPL_E_INVALID;
    const unsigned f = cfg->flags;
    if ((f & MPL_F_POS3D_TO_RAYS) && !(f & MPL_F_RAYS_TOKEN)) return MPL_E_UNSUPPORTED;  // reference itself fails (:483)
    if ((f & MPL_F_POS3D_TO_RAYS) && (f & MPL_F_POS3D_SPATIAL)) return MPL_E_UNSUPPORTED;
    SptParams p;
    const bool needs_rays = (f & MPL_F_RAYS_TOKEN) || !(f & MPL_F_POS3D_LEARN);
    for (int v = 0; v < MPL_MAX_VIEWS; ++v) {
        const bool on = v < cfg->num_views;
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
    p.xs = xs;
    p.B = in->batch; p.V = cfg->num_views; p.in_ch = cfg->in_chans;
    p.flags = f;
    p.c3 = (f & MPL_F_POS3D_TO_RAYS) ? 2 * SD : SD;
    // the phase ablations (garbage results) exist in laboratory builds only: tools/build_variants.sh -f spt.hip
    static const int abl = lab_getenv("MPL_SPT_ABL") ? atoi(lab_getenv("MPL_SPT_ABL")) : 0;
    p.abl = abl;
    {
        int dev = 0;
        p.err_host = hipGetDevice(&dev) == hipSuccess ? device_error_word(dev) : nullptr;
    }
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
    const int form = spt_form(cfg, in->batch, use_packed, cus, &p.spw);
    if (form < 0) return form;
    const int grid = cfg->num_views * ((in->batch + p.spw - 1) / p.spw);
    ProfScope prof(MPL_K_SPT, s);
    return form == MPL_SPT_PACKED ? launch_spt_packed(p, p.spw, grid, s) : launch_spt_native(p, form, grid, s);
}


}  // namespace mpl
