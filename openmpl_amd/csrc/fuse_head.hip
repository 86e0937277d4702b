// Tail of the forward: strip ray features, View_norm, learned weighted mean over views, head.
//
// Reference (MPL/lib/models/multiview_mpl.py):
//   :425-434  ray-token strip  -- token variant keeps [2][J][d] half 0, feature variant keeps [J][2d][:d]
//   :439      View_norm = LayerNorm(J*d, eps 1e-6) per (b, v) row
//   :445      weighted_mean = Conv1d(V -> 1, k = 1):  y[f] = sum_v w_v * xn[v][f] + bias
//   :521-523  head = LayerNorm(J*d, eps 1e-5) -> Linear(J*d, 3J) -> view(B, J, 3)
// Four poses per 256-thread workgroup (one wave each), the head Linear batched over the four.
#include "fuse_head.hpp"

namespace mpl {

// FH_POSES poses (= waves) per workgroup, one WAVE per pose for everything that is per pose (View_norm statistics, weighted
// mean over views, head LayerNorm: wave reductions only, no block barrier: fuse_head.hpp fh_pose), then the head Linear for all
// of them at once (fh_linear).  Round 1 ran one workgroup per pose: a chain of ~10 dependent global-memory round trips and 51 x 4
// re-reads of the 111 kB head weight per workgroup made it 45-54 us for 8.9 MB of input; this form is ~4 round trips.
// FH_POSES = 4 (256 threads).  Eight poses per 512-thread workgroup (half the workgroups, half the copies of the 111-kB head weight
// through L2) measured 20.3 against 20.9 us at B = 1024 (profiles/r06_ab_fh8.txt): the kernel is a chain of memory round trips, not
// bytes -- not kept.
template <int FH_POSES>
__global__ __launch_bounds__(64 * FH_POSES) void fuse_head_kernel(const float* __restrict__ x, int B, const FhParams p, float* __restrict__ out,
                                                                  float* __restrict__ y_out, const unsigned* __restrict__ err_ws) {
    extern __shared__ __attribute__((aligned(1024))) float fh_smem[];
    float* hws = fh_smem;                                    // the head weight [n_out][E], staged by LDS-DMA
    float (*y)[kMaxE] = reinterpret_cast<float (*)[kMaxE]>(fh_smem + FH_W_FLOATS);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the block stack of this call reported a lost hand-off: its rows are not to be trusted -- the result is NaN, never a
    // plausible-looking pose (the host raises on the next call: MPL_E_DEVICE).  The word was written (if at all) by the
    // previous kernel of this stream; requested now, used at the very end.
    const unsigned poisoned = err_ws ? __hip_atomic_load(err_ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    if (!y_out) fh_stage_weight(p, hws, wave, lane, FH_POSES);       // lands while the waves normalise and fuse their poses
    const int b = blockIdx.x * FH_POSES + wave;
    if (b < B)
        fh_pose<false>(p, x + (size_t)b * p.V * p.Df, lane, y[wave], y_out ? y_out + (size_t)b * p.E : nullptr, poisoned != 0u);
    if (y_out) return;
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int np = (B - blockIdx.x * FH_POSES) < FH_POSES ? (B - blockIdx.x * FH_POSES) : FH_POSES;
    const int b0 = blockIdx.x * FH_POSES;
    fh_linear(p, hws, y, np, tid, 64 * FH_POSES, out, poisoned != 0u, [&](int ps) { return b0 + ps; });
}

// ------------------------------------------------------------------------------------------
// The same tail for any E = J*d up to 4096 (shapes fh_params refuses): one 256-thread workgroup per pose.  The View_norm-ed rows
// of the V views are accumulated (weighted mean, Conv1d form) into an LDS row of E floats that each thread owns a strided part
// of; then either that feature goes to y_out (non-default heads) or head[0] LayerNorm (eps 1e-5) and head[1] Linear(E -> 3J)
// follow, the Linear as one wave per output with lanes striding over the features (coalesced reads of the weight row).
constexpr int FA_THR = 256, FA_MAX_E = 4096;

__device__ __forceinline__ float fa_block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum(v);
    __syncthreads();                       // red is reused by consecutive reductions
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(FA_THR) void fuse_any_kernel(const float* __restrict__ x, const FhParams p, float* __restrict__ out,
                                                          float* __restrict__ y_out, const unsigned* __restrict__ err_ws) {
    extern __shared__ __attribute__((aligned(16))) float fa_smem[];
    float* y = fa_smem;                    // [E]
    float* red = fa_smem + p.E;            // [4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, E = p.E, d = p.d;
    const int b = blockIdx.x;
    const bool poisoned = err_ws && __hip_atomic_load(err_ws, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    auto src = [&](int f) { return p.strip_mode == 1 ? (f / d) * 2 * d + (f % d) : f; };
    for (int f = tid; f < E; f += FA_THR) y[f] = 0.f;
    for (int v = 0; v < p.V; ++v) {        // View_norm (:439) + Conv1d weighted mean over views (:445)
        const float* xr = x + ((size_t)b * p.V + v) * p.Df;
        float s = 0.f;
        for (int f = tid; f < E; f += FA_THR) s += xr[src(f)];
        const float mean = fa_block_sum(s, red) / (float)E;
        float ss = 0.f;
        for (int f = tid; f < E; f += FA_THR) {
            const float t = xr[src(f)] - mean;
            ss += t * t;
        }
        const float rstd = 1.0f / sqrtf(fa_block_sum(ss, red) / (float)E + 1e-6f);
        const float wv = p.wm_w[v];
        for (int f = tid; f < E; f += FA_THR) y[f] = fmaf(wv, (xr[src(f)] - mean) * rstd * p.vn_w[f] + p.vn_b[f], y[f]);
    }
    const float wb = p.wm_b[0];
    if (y_out) {
        for (int f = tid; f < E; f += FA_THR) y_out[(size_t)b * E + f] = poisoned ? __builtin_nanf("") : y[f] + wb;
        return;
    }
    float s = 0.f;                         // head[0] LayerNorm (eps 1e-5), two-pass
    for (int f = tid; f < E; f += FA_THR) {
        y[f] += wb;
        s += y[f];
    }
    const float mean = fa_block_sum(s, red) / (float)E;
    float ss = 0.f;
    for (int f = tid; f < E; f += FA_THR) {
        const float t = y[f] - mean;
        ss += t * t;
    }
    const float rstd = 1.0f / sqrtf(fa_block_sum(ss, red) / (float)E + 1e-5f);
    for (int f = tid; f < E; f += FA_THR) y[f] = (y[f] - mean) * rstd * p.hl_w[f] + p.hl_b[f];
    __syncthreads();
    for (int o = wave; o < p.n_out; o += FA_THR / 64) {      // head[1] Linear (:521)
        const float* wr = p.hw + (size_t)o * E;
        float a = 0.f;
        for (int f = lane; f < E; f += 64) a = fmaf(y[f], wr[f], a);
        a = wave_sum(a);
        if (lane == 0) out[(size_t)b * p.n_out + o] = poisoned ? __builtin_nanf("") : a + p.hb[o];
    }
}

static int launch_fuse_any(const mpl_config* cfg, const mpl_weights* w, const float* x, int batch, float* out, float* y_out,
                           const unsigned* err_ws, hipStream_t s) {
    const int J = cfg->num_joints, d = cfg->dim, V = cfg->num_views, E = J * d;
    if (E < 1 || E > FA_MAX_E || V < 1 || V > MPL_MAX_VIEWS) return MPL_E_UNSUPPORTED;
    if (!x || !w->view_norm_w || !w->view_norm_b || !w->wmean_w || !w->wmean_b) return MPL_E_INVALID;
    if (!y_out && (!out || !w->head_ln_w || !w->head_ln_b || !w->head_w || !w->head_b)) return MPL_E_INVALID;
    int strip = 0;
    if (cfg->flags & MPL_F_POS3D_TO_RAYS) strip = 1;           // :430-434 (takes precedence, elif order)
    else if (cfg->flags & MPL_F_RAYS_TOKEN) strip = 2;         // :425-429
    const FhParams p{w->view_norm_w, w->view_norm_b, w->wmean_w, w->wmean_b, w->head_ln_w, w->head_ln_b, w->head_w, w->head_b,
                     V, mpl_fpt_width(cfg), E, d, strip, 3 * J};
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(fuse_any_kernel, dim3(batch), dim3(FA_THR), (size_t)(E + 4) * sizeof(float), s, x, p, out, y_out, err_ws);
    return hip_check_launch();
}

int launch_fuse_head(const mpl_config* cfg, const mpl_weights* w, const float* x, int batch, float* out, float* y_out,
                     const unsigned* err_ws, hipStream_t s) {
    FhParams p;
    if (batch <= 0) return MPL_E_UNSUPPORTED;
    if (!fh_params(cfg, w, &p)) return launch_fuse_any(cfg, w, x, batch, out, y_out, err_ws, s);
    constexpr int poses = 4;
    constexpr int LDS = (FH_W_FLOATS + poses * kMaxE) * 4;
    if (int rc = kernel_lds_once<fuse_head_kernel<poses>>(LDS)) return rc;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(fuse_head_kernel<poses>, dim3((batch + poses - 1) / poses), dim3(64 * poses), LDS, s, x, batch, p, out, y_out, err_ws);
    return hip_check_launch();
}

}  // namespace mpl
