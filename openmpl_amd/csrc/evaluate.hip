// Device-resident evaluator of a whole validation run (the second half of SURVEY.md 8f rank f3): everything validate() does
// on the host after `model(...)`, fed once per batch on the forward's stream, read back once at the end of the run.
//
// Reference (MPL/lib/core/): function_mpl.py:387-399 (criterion + AverageMeter), :474-494 (de-normalisation, all_preds /
// all_gts / all_3d_confs), :612-634 and :670-785 evaluate() (metre factor, relative mode, conf_3d mask, calc_mpjpe,
// calc_distance_per_dim, per action), loss.py:39-57 MPJPE, :59-104 L1 / MSE, :110-124 Weighted_MPJPE, :127-146 MPJPE_KADKHODA.
//
// eval_accumulate_kernel: a grid of workgroups, each owning a contiguous slice of the batch; thread = (joint, slice of the
// slice) accumulating in fp64, folded through LDS in a fixed order (as metrics.hip) into per-workgroup partials.
// eval_fold_kernel: adds the partials to the state by workgroup index.  No floating-point atomics anywhere: a run is bitwise
// reproducible.  eval_report_kernel: the state -> what evaluate() returns, per pass (absolute, relative) and group.
// Element-wise arithmetic is fp32 in the reference's own order (no contraction), so that only the reductions differ from numpy.
#include "common.hpp"

namespace mpl {

namespace {

constexpr int EV_ACC = 16;     // per (group, selected joint): 8 per pass -- 0 error sum, 1-3 |e| sums, 4-6 non-NaN counts, 7 samples
constexpr int EV_WGS = 32;     // most workgroups of one accumulate launch (the partial area of the state is sized for it)
constexpr int EV_SPW = 64;     // fewest samples per workgroup

struct EvalHeader {
    unsigned poisoned;          // set when a batch arrived while the device's error word was set: every report is NaN
    unsigned pad;
    unsigned long long n_samples;
    double crit[5];             // AverageMeter sums: loss, 3 per-axis values, weight (function_mpl.py:396-399)
    double reserved[9];
};
static_assert(sizeof(EvalHeader) == 128, "state header");

__host__ __device__ inline size_t ev_acc_doubles(int n_sel, int n_groups) { return (size_t)n_groups * n_sel * EV_ACC; }
__host__ __device__ inline size_t ev_partial_doubles(int n_sel, int n_groups) { return ev_acc_doubles(n_sel, n_groups) + 4; }

inline int ev_workgroups(int B) {
    const int g = (B + EV_SPW - 1) / EV_SPW;
    return g < EV_WGS ? g : EV_WGS;
}

struct EvalArgs {
    const float *out, *x1, *x2, *tgt, *wgt, *conf;
    const int32_t* gid;
    float *keep_pred, *keep_tgt;
    long long keep_cap;
    int B, J, spw;
};

__global__ __launch_bounds__(256) void eval_accumulate_kernel(EvalArgs a, mpl_eval_options o, char* __restrict__ state,
                                                               const unsigned* __restrict__ dev_err) {
#pragma clang fp contract(off)
    __shared__ double acc[256 * EV_ACC];
    __shared__ float nrm[64 * 64];          // MPJPE with weight_axis: the (B,J) norms of the one workgroup
    __shared__ unsigned present[MPL_EVAL_MAX_GROUPS];
    const int tid = threadIdx.x;
    EvalHeader* hdr = reinterpret_cast<EvalHeader*>(state);
    // the rule of metrics.hip: NaN poses of a failed forward would be skipped by nansum / nanmean and score as zero error
    if (dev_err && __hip_atomic_load(dev_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) {
        if (tid == 0) hdr->poisoned = 1u;
        return;
    }
    const int J = a.J, S = o.n_sel, G = o.n_groups;
    const int JT = J > S ? J : S, NS = 256 / JT;
    const int k = tid % JT, s = tid / JT;
    const int b0 = blockIdx.x * a.spw, b1 = min(a.B, b0 + a.spw);
    double* part = reinterpret_cast<double*>(state + sizeof(EvalHeader)) + ev_acc_doubles(S, G) +
                   (size_t)blockIdx.x * ev_partial_doubles(S, G);
    const unsigned long long seen = hdr->n_samples;     // written by the fold of the batch before this one

    // ---- criterion on the raw tensors (all J joints) + the kept de-normalised poses
    double c[4] = {0, 0, 0, 0};
    if (tid < MPL_EVAL_MAX_GROUPS) present[tid] = 0u;
    if (k < J && s < NS) {
        for (int b = b0 + s; b < b1; b += NS) {
            const size_t at = ((size_t)b * J + k) * 3;
            float e[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) e[d] = a.out[at + d] - a.tgt[at + d];
            float term = 0.f;
            switch (o.criterion) {
                case MPL_CRIT_MPJPE:
                case MPL_CRIT_WEIGHTED_MPJPE: {
                    float n2 = 0.f;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float ew = o.has_weight_axis && o.criterion == MPL_CRIT_MPJPE ? e[d] * o.weight_axis[d] : e[d];
                        n2 += ew * ew;
                        c[1 + d] += fabsf(e[d]);
                    }
                    term = sqrtf(n2);
                    if (o.criterion == MPL_CRIT_WEIGHTED_MPJPE) term = a.wgt[(size_t)b * J + k] * term;      // loss.py:124
                    else if (o.has_weight_axis) nrm[(b - b0) * 64 + k] = term;                             // loss.py:56, below
                    break;
                }
                case MPL_CRIT_L1:            // loss.py:74-79
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float v = fabsf(e[d]);
                        term += o.has_weight_axis ? v * o.weight_axis[d] : v;
                        c[1 + d] += v;
                    }
                    break;
                case MPL_CRIT_MSE:           // loss.py:99-104: the per-axis values are squared errors too
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const float v = e[d] * e[d];
                        term += o.has_weight_axis ? v * o.weight_axis[d] : v;
                        c[1 + d] += v;
                    }
                    break;
                default: {                   // MPJPE_KADKHODA, loss.py:139-146: F.pairwise_distance adds eps = 1e-6 to the difference
                    const float* xs[3] = {a.x1, a.x2, a.out};
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        float n2 = 0.f;
#pragma unroll
                        for (int d = 0; d < 3; ++d) {
                            const float v = xs[i][at + d] - a.tgt[at + d] + 1e-6f;
                            n2 += v * v;
                        }
                        const float dist = sqrtf(n2);
                        term += dist * dist;
                    }
#pragma unroll
                    for (int d = 0; d < 3; ++d) c[1 + d] += fabsf(e[d]);
                }
            }
            c[0] += term;
            if (a.keep_pred && (long long)(seen + b) < a.keep_cap) {          // function_mpl.py:476-491, before all_preds[:, u, :]
                const size_t kat = ((size_t)(seen + b) * J + k) * 3;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    a.keep_pred[kat + d] = a.out[at + d] * o.scale[d] + o.offset[d];
                    a.keep_tgt[kat + d] = a.tgt[at + d] * o.scale[d] + o.offset[d];
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[tid * EV_ACC + q] = c[q];
    __syncthreads();
    if (a.gid && tid < b1 - b0) {           // spw <= 256: which groups this slice holds (any order, every writer stores 1)
        for (int b = b0 + tid; b < b1; b += 256) {
            const int g = a.gid[b];
            if (g >= 1 && g < G) present[g] = 1u;
        }
    }
    double cj[4] = {0, 0, 0, 0};
    if (tid < J)                            // slices in order
        for (int q = 0; q < NS; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) cj[i] += acc[(q * JT + tid) * EV_ACC + i];
    __syncthreads();
    if (tid < J)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[tid * EV_ACC + i] = cj[i];
    __syncthreads();
    if (o.criterion == MPL_CRIT_MPJPE && o.has_weight_axis) {
        // loss.py:56 `w * norm`: w (B,J,1) against norm (B,J) broadcasts to (B, max(B,J), J) with element [a,b,c] = w[a,b] * norm[b,c]
        // -- defined for B == 1, J == 1 or B == J only (anything else raises in the reference and is refused by the host side);
        // its sum is sum_b (sum_a w[a,b]) (sum_c norm[b,c]).  One workgroup holds the whole batch (B <= 64).
        const int M = a.B > J ? a.B : J;
        double prod = 0;
        if (tid < M) {
            const int bw = J > 1 ? tid : 0, bn = a.B > 1 ? tid : 0;
            double cs = 0, rs = 0;
            for (int q = 0; q < a.B; ++q) cs += (double)a.wgt[(size_t)q * J + bw];
            for (int q = 0; q < J; ++q) rs += (double)nrm[bn * 64 + q];
            prod = cs * rs;
        }
        __syncthreads();
        if (tid < 64) acc[tid * EV_ACC + 4] = prod;
        __syncthreads();
    }
    if (tid == 0) {                         // joints in order
        double t[4] = {0, 0, 0, 0};
        for (int q = 0; q < J; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) t[i] += acc[q * EV_ACC + i];
        if (o.criterion == MPL_CRIT_MPJPE && o.has_weight_axis) {
            t[0] = 0;
            const int M = a.B > J ? a.B : J;
            for (int q = 0; q < M; ++q) t[0] += acc[q * EV_ACC + 4];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) part[ev_acc_doubles(S, G) + i] = t[i];
    }
    __syncthreads();

    // ---- evaluate(): one walk of the slice per group (group 0 = every sample)
    const int src = k < S ? o.sel[k] : 0, root = o.sel[0];
    for (int g = 0; g < G; ++g) {
        double* pg = part + (size_t)g * S * EV_ACC;
        if (g > 0 && !present[g]) {         // uniform over the workgroup
            for (int i = tid; i < S * EV_ACC; i += 256) pg[i] = 0.0;
            continue;
        }
        double v[EV_ACC] = {};
        if (k < S && s < NS) {
            for (int b = b0 + s; b < b1; b += NS) {
                if (g > 0 && a.gid[b] != g) continue;
                const size_t at = ((size_t)b * J + src) * 3, at0 = ((size_t)b * J + root) * 3;
                const bool gone = a.conf && !(a.conf[(size_t)b * J + src] > 0.f);       // evaluate():683-684 `conf_3d <= 0`
                const bool gone0 = a.conf && !(a.conf[(size_t)b * J + root] > 0.f);
                float abs2 = 0.f, rel2 = 0.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    // function_mpl.py:476-488, then evaluate():674-676
                    const float P = (a.out[at + d] * o.scale[d] + o.offset[d]) * o.metre_factor;
                    const float T = (a.tgt[at + d] * o.scale[d] + o.offset[d]) * o.metre_factor;
                    const float P0 = (a.out[at0 + d] * o.scale[d] + o.offset[d]) * o.metre_factor;
                    const float T0 = (a.tgt[at0 + d] * o.scale[d] + o.offset[d]) * o.metre_factor;
                    const float nan = __builtin_nanf("");
                    // absolute pass: calc_mpjpe(gt, pred) then calc_distance_per_dim(pred, gt)
                    const float ea = gone ? nan : T - P;
                    if (!isnan(ea)) {
                        abs2 += ea * ea;
                        v[1 + d] += fabsf(ea);
                        v[4 + d] += 1.0;
                    }
                    // relative pass: evaluate():678-680 subtracts the root, :682-684 masks, calc_mpjpe 'relative' subtracts the
                    // (now zero, or NaN when the root is masked) root AGAIN; calc_distance_per_dim sees the once-subtracted poses
                    const float Tq = gone ? nan : T - T0, Pq = gone ? nan : P - P0;
                    const float rT = gone0 ? nan : T0 - T0, rP = gone0 ? nan : P0 - P0;
                    const float ed = Pq - Tq;
                    if (!isnan(ed)) {
                        v[8 + 1 + d] += fabsf(ed);
                        v[8 + 4 + d] += 1.0;
                    }
                    const float er = (Tq - rT) - (Pq - rP);
                    if (!isnan(er)) rel2 += er * er;
                }
                v[0] += sqrtf(abs2);
                v[8] += sqrtf(rel2);
                v[7] += 1.0;
                v[15] += 1.0;
            }
        }
#pragma unroll
        for (int q = 0; q < EV_ACC; ++q) acc[tid * EV_ACC + q] = v[q];
        __syncthreads();
        if (tid < S) {
            double t[EV_ACC] = {};
            for (int q = 0; q < NS; ++q)
#pragma unroll
                for (int i = 0; i < EV_ACC; ++i) t[i] += acc[(q * JT + tid) * EV_ACC + i];
#pragma unroll
            for (int i = 0; i < EV_ACC; ++i) pg[tid * EV_ACC + i] = t[i];
        }
        __syncthreads();
    }
}

// one workgroup per group: partials in workgroup order, then into the state; workgroup 0 also closes the batch's AverageMeter step
__global__ __launch_bounds__(256) void eval_fold_kernel(char* __restrict__ state, int n_sel, int n_groups, int n_wgs, int B, int J,
                                                         int n_views, double crit_div) {
    EvalHeader* hdr = reinterpret_cast<EvalHeader*>(state);
    if (hdr->poisoned) return;
    double* accs = reinterpret_cast<double*>(state + sizeof(EvalHeader));
    const double* parts = accs + ev_acc_doubles(n_sel, n_groups);
    const size_t stride = ev_partial_doubles(n_sel, n_groups);
    const int g = blockIdx.x;
    for (int i = threadIdx.x; i < n_sel * EV_ACC; i += 256) {
        const size_t at = (size_t)g * n_sel * EV_ACC + i;
        double t = 0;
        for (int w = 0; w < n_wgs; ++w) t += parts[(size_t)w * stride + at];
        accs[at] += t;
    }
    if (g == 0 && threadIdx.x < 4) {
        double t = 0;
        for (int w = 0; w < n_wgs; ++w) t += parts[(size_t)w * stride + ev_acc_doubles(n_sel, n_groups) + threadIdx.x];
        const double n = (double)n_views * B;                  // `len(input) * input[0].size(0)`
        const double div = threadIdx.x == 0 ? crit_div : (double)B * J;
        hdr->crit[threadIdx.x] += t / div * n;
        if (threadIdx.x == 0) {
            hdr->crit[4] += n;
            hdr->n_samples += (unsigned long long)B;
        }
    }
}

// grid (n_groups, 2 passes); report: 8 doubles of header, then per (pass, group) pjpe[S], mpjpe, dist[S][3], dist_mean[3], samples
__global__ __launch_bounds__(64) void eval_report_kernel(const char* __restrict__ state, int n_sel, int n_groups,
                                                          unsigned long long skip_mask, double* __restrict__ rep) {
    __shared__ double sh[64][4];
    const EvalHeader* hdr = reinterpret_cast<const EvalHeader*>(state);
    const double* accs = reinterpret_cast<const double*>(state + sizeof(EvalHeader));
    const int g = blockIdx.x, pass = blockIdx.y, tid = threadIdx.x, S = n_sel;
    const bool bad = hdr->poisoned != 0u;
    const double nan = __builtin_nan("");
    double* r = rep + 8 + ((size_t)pass * n_groups + g) * (4 * S + 5);
    if (g == 0 && pass == 0 && tid < 8) {
        double v = 0;
        if (tid < 4) v = bad ? nan : hdr->crit[tid] / hdr->crit[4];          // AverageMeter.avg; nothing fed: NaN
        else if (tid == 4) v = (double)hdr->n_samples;
        else if (tid == 5) v = bad ? 1.0 : 0.0;
        rep[tid] = v;
    }
    if (tid < S) {
        const double* t = accs + ((size_t)g * S + tid) * EV_ACC + pass * 8;
        sh[tid][0] = bad ? nan : t[0] / t[7];                                 // calc_mpjpe: mean over samples
#pragma unroll
        for (int d = 0; d < 3; ++d) sh[tid][1 + d] = bad ? nan : t[1 + d] / t[4 + d];      // np.nanmean: 0 / 0 = NaN
        r[tid] = sh[tid][0];
#pragma unroll
        for (int d = 0; d < 3; ++d) r[S + 1 + tid * 3 + d] = sh[tid][1 + d];
    }
    __syncthreads();
    if (tid == 0) {
        double m = 0, dm[3] = {0, 0, 0};
        int kept = 0;              // evaluate.py:101-104, :110-113: np.delete on the SELECTED joints, from the mean only
        for (int q = 0; q < S; ++q) {
            if (!((skip_mask >> q) & 1ull)) {
                m += sh[q][0];
                ++kept;
            }
            for (int d = 0; d < 3; ++d) dm[d] += sh[q][1 + d];
        }
        r[S] = m / kept;
        for (int d = 0; d < 3; ++d) r[S + 1 + 3 * S + d] = dm[d] / S;
        r[4 * S + 4] = accs[(size_t)g * S * EV_ACC + 7];
    }
}

int ev_shape_check(int n_sel, int n_groups) {
    if (n_sel < 1 || n_groups < 1) return MPL_E_INVALID;
    if (n_sel > 64 || n_groups > MPL_EVAL_MAX_GROUPS) return MPL_E_UNSUPPORTED;
    return MPL_OK;
}

}  // namespace

size_t eval_state_bytes(int n_sel, int n_groups) {
    if (ev_shape_check(n_sel, n_groups)) return 0;
    return sizeof(EvalHeader) + (ev_acc_doubles(n_sel, n_groups) + EV_WGS * ev_partial_doubles(n_sel, n_groups)) * sizeof(double);
}

int launch_eval_reset(void* state, int n_sel, int n_groups, hipStream_t s) {
    if (int rc = ev_shape_check(n_sel, n_groups)) return rc;
    if (!state) return MPL_E_INVALID;
    // all-zero bytes are 0.0 and a clean header; the partial area is written before it is read
    return hipMemsetAsync(state, 0, sizeof(EvalHeader) + ev_acc_doubles(n_sel, n_groups) * sizeof(double), s) == hipSuccess ? MPL_OK
                                                                                                                             : MPL_E_LAUNCH;
}

int launch_eval_accumulate(void* state, const mpl_eval_options* o, const float* out, const float* x1, const float* x2,
                           const float* tgt, const float* wgt, const float* conf, const int32_t* gid, int B, int J, float* keep_pred,
                           float* keep_tgt, long long keep_cap, hipStream_t s) {
    if (!state || !o || !out || !tgt || B <= 0 || J <= 0) return MPL_E_INVALID;
    if (J > 64) return MPL_E_UNSUPPORTED;
    if (int rc = ev_shape_check(o->n_sel, o->n_groups)) return rc;
    if (o->criterion < MPL_CRIT_MPJPE || o->criterion > MPL_CRIT_MPJPE_KADKHODA || o->n_views < 1) return MPL_E_INVALID;
    for (int i = 0; i < o->n_sel; ++i)
        if (o->sel[i] >= J) return MPL_E_INVALID;
    const bool wa = o->criterion == MPL_CRIT_MPJPE && o->has_weight_axis;
    if ((o->criterion == MPL_CRIT_WEIGHTED_MPJPE || wa) && !wgt) return MPL_E_INVALID;
    if (o->criterion == MPL_CRIT_MPJPE_KADKHODA && (!x1 || !x2)) return MPL_E_INVALID;
    if ((keep_pred != nullptr) != (keep_tgt != nullptr) || (keep_pred && keep_cap <= 0)) return MPL_E_INVALID;
    if (o->n_groups > 1 && !gid) return MPL_E_INVALID;
    double div = (double)B * J;
    if (wa) {      // loss.py:56 broadcasts only these shapes; the whole batch sits in one workgroup
        if (!(B == 1 || J == 1 || B == J)) return MPL_E_INVALID;
        if (B > EV_SPW) return MPL_E_UNSUPPORTED;
        div = (double)B * (B > J ? B : J) * J;
    }
    int dev = 0;
    const unsigned* dev_err = hipGetDevice(&dev) == hipSuccess ? device_error_word(dev) : nullptr;
    const int wgs = ev_workgroups(B);
    EvalArgs a{out, x1, x2, tgt, wgt, conf, o->n_groups > 1 ? gid : nullptr, keep_pred, keep_tgt, keep_cap, B, J, (B + wgs - 1) / wgs};
    {
        ProfScope prof(MPL_K_FUSE_HEAD, s);
        hipLaunchKernelGGL(eval_accumulate_kernel, dim3(wgs), dim3(256), 0, s, a, *o, reinterpret_cast<char*>(state), dev_err);
    }
    if (int rc = hip_check_launch()) return rc;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(eval_fold_kernel, dim3(o->n_groups), dim3(256), 0, s, reinterpret_cast<char*>(state), o->n_sel, o->n_groups, wgs, B,
                       J, o->n_views, div);
    return hip_check_launch();
}

int eval_report_doubles(int n_sel, int n_groups) {
    if (ev_shape_check(n_sel, n_groups)) return 0;
    return 8 + 2 * n_groups * (4 * n_sel + 5);
}

int launch_eval_report(const void* state, int n_sel, int n_groups, uint64_t skip_mask, double* rep, hipStream_t s) {
    if (int rc = ev_shape_check(n_sel, n_groups)) return rc;
    if (!state || !rep) return MPL_E_INVALID;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(eval_report_kernel, dim3(n_groups, 2), dim3(64), 0, s, reinterpret_cast<const char*>(state), n_sel, n_groups,
                       (unsigned long long)skip_mask, rep);
    return hip_check_launch();
}

}  // namespace mpl
