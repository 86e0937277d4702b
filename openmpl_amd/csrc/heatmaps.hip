// Detector heatmaps decoded into pixel detections (and, with cameras, into the model's inputs) on the device: the step in front
// of prepare_inputs_kernel, which the reference runs on the host per (sample, joint) in Python.
//
// Reference (MPL/lib/core/inference.py): get_max_preds :22-50 -- argmax / amax over the H*W values, x = idx % W, y = idx / W, both
// times (maxval > 0); get_final_preds :53-81 -- with TEST.POST_PROCESS a quarter-pixel shift towards the higher neighbour where
// 1 < x < W-1 and 1 < y < H-1, then transform_preds (MPL/lib/utils/transforms.py:51-94) with rot = 0 back to the image.
// The affine fit of transform_preds is written in closed form: k = scale_x * 200 / W, pixel = center + (coord - (W/2, H/2)) * k, in
// fp64 on the fp32 inputs, rounded once.  The one deviation: the reference rounds the three anchor points of the fit to float32
// before it solves, the closed form does not (a few fp32 ulps, more where the pixel is a cancelled difference).
//
// One launch.  decode_kernel<DT, 1>: one wave per heatmap, four heatmaps per 256-thread workgroup; decode_kernel<DT, 4>: the four
// waves of a workgroup share one heatmap (maps of 64 KiB or more, decode_waves_per_map) and merge through LDS.  A map whose base
// and byte size are multiples of 16 is read with 16-byte loads, sixteen of them in flight per lane before the first compare;
// every other map takes the element-wise path.  Each lane keeps (value, index) under strict > in increasing index order and
// flags NaNs; a flagged lane (rare) looks up its first NaN.  Lanes and waves merge by one total order -- NaN above everything,
// then the value (-0 == 0), then the lower index -- so the result is np.argmax's whatever the reduction tree, and both forms
// and both paths give identical outputs.  No atomics, no scratch; 16-bit maps are widened exactly.
//
// Sub-pixel decoding (mpl_decode_heatmaps_ex) replaces the quarter-cell shift by a refinement of the integer peak, chosen by the
// template parameter RF after the scan, which it does not touch: MPL_REFINE_GAUSSIAN, the log-quadratic fit through the peak and
// its neighbours on each axis, on the finishing lane; MPL_REFINE_CENTROID, the thresholded window centroid that the reference's
// find_tensor_peak_batch (inference.py:84-134) means to compute, spread over the finishing wave.  RF = MPL_REFINE_NONE compiles
// to the kernels as they were.
#include "common.hpp"
#include "views.hpp"

namespace mpl {

struct DecodeParams : HeatmapTable {
    ViewOutputs out;
    const float* center;             // (B,V,2) or null
    const float* scale;              // (B,V,2) or null; component 1 is not read
    const double* cams;              // device (V,16) or null
    float* pixels;                   // (B,V,J,2)
    float* conf;                     // (B,V,J)
    float* coords;                   // (B,V,J,2) or null
    int total;                       // B * V * J
    int post;
    double w, h;
    int norm_in, norm_cam;
    int radius;                      // MPL_REFINE_CENTROID: the window is (2 radius + 1)^2 cells
    double threshold;                // MPL_REFINE_CENTROID: values not above it count as 0
};

constexpr int DECODE_EMPTY = 0x7fffffff;     // index of a lane that has seen no value above -inf

// The launch rule: a map of 64 KiB or more is streamed by the four waves of a workgroup, a smaller one by one wave.
inline int decode_waves_per_map(size_t map_bytes) { return map_bytes >= 65536 ? 4 : 1; }

template <int DT> struct HmElem { static constexpr int size = DT == MPL_HM_F32 ? 4 : 2, per_chunk = 16 / size; };

template <int DT>
__device__ __forceinline__ float hm_load(const void* base, size_t i) { return hm_fetch(base, i, DT); }

template <int DT>
__device__ __forceinline__ void hm_unpack(const uint4& q, float (&v)[HmElem<DT>::per_chunk]) {
    const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (DT == MPL_HM_F32) {
            v[k] = __uint_as_float(d[k]);
        } else if (DT == MPL_HM_BF16) {
            v[2 * k] = __uint_as_float(d[k] << 16);
            v[2 * k + 1] = __uint_as_float(d[k] & 0xffff0000u);
        } else {
            v[2 * k] = hm_widen16<DT>(d[k] & 0xffffu);
            v[2 * k + 1] = hm_widen16<DT>(d[k] >> 16);
        }
    }
}

// U chunks of one lane, NT chunks apart, all loaded before the first compare.  rel counts elements from the lane's first one.
// odd collects x * 0: it turns NaN once the lane has seen a NaN or an infinity, in one multiply-add per value and no compare mask.
template <int DT, int NT, int U>
__device__ __forceinline__ void hm_scan(const uint4* q, int rel0, float& cur, int& rel, float& odd) {
    constexpr int E = HmElem<DT>::per_chunk;
    uint4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = q[(size_t)u * NT];
    __builtin_amdgcn_sched_barrier(0);      // every load is issued before the first compare: U x 16 bytes in flight per lane
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float v[E];
        hm_unpack<DT>(r[u], v);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (v[e] > cur) { cur = v[e]; rel = rel0 + u * NT * E + e; }
            odd = fmaf(v[e], 0.0f, odd);
        }
    }
}

// a is ahead of b: NaN above everything, then the value, then the lower index
__device__ __forceinline__ bool hm_ahead(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

__device__ __forceinline__ float hm_quarter(float hi, float lo) {      // 0.25 * np.sign(hi - lo), by comparison
    if (hi != hi || lo != lo) return __uint_as_float(0x7fc00000u);
    return hi > lo ? 0.25f : (hi < lo ? -0.25f : 0.0f);
}

// ---- sub-pixel refinement of the integer peak (mpl_decode_heatmaps_ex), after the scan and the merge; RF is MPL_REFINE_*.

// MPL_REFINE_GAUSSIAN, one axis: the log-quadratic fit through the peak f0 (l0 = ln f0) and its two neighbours `stride` elements
// away; c is the peak's coordinate on the axis of n cells.  Exact for a Gaussian of any sigma; within +/-0.5 as f0 is the maximum.
template <int DT>
__device__ __forceinline__ double hm_log_quadratic(const char* base, size_t at, size_t stride, int c, int n, double l0) {
    if (c == 0 || c == n - 1) return 0.0;
    const float fm = hm_load<DT>(base, at - stride), fp = hm_load<DT>(base, at + stride);
    if (!(fm > 0.0f && fm < INFINITY && fp > 0.0f && fp < INFINITY)) return 0.0;
    const double a = l0 - log((double)fp), b = l0 - log((double)fm);
    return a + b == 0.0 ? 0.0 : (b - a) / (2.0 * (a + b));
}

// MPL_REFINE_CENTROID: the thresholded centroid of the window about the peak (px, py), relative to the peak.  Called by all 64
// lanes of the finishing wave with the same arguments: cell t = (j + r) * (2r + 1) + (i + r) goes to lane t % 64, a lane adds its
// cells in increasing t, the lanes add up pairwise -- one order, whatever the form of the kernel.  Every lane returns the sums.
template <int DT>
__device__ __forceinline__ void hm_centroid(const char* base, int px, int py, int W, int H, int r, double threshold, int lane, double& dx,
                                            double& dy) {
    const int n = 2 * r + 1;
    double sw = 0.0, sx = 0.0, sy = 0.0;
    for (int t = lane; t < n * n; t += 64) {
        const int i = t % n - r, j = t / n - r, x = px + i, y = py + j;
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        const double w = (double)hm_load<DT>(base, (size_t)y * W + x);
        if (w > threshold) { sw += w; sx += w * (double)i; sy += w * (double)j; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sw += __shfl_xor(sw, off, 64);
        sx += __shfl_xor(sx, off, 64);
        sy += __shfl_xor(sy, off, 64);
    }
    const double S = sw + 2.22e-16;
    dx = sx / S;
    dy = sy / S;
}

template <int DT, int WAVES, int RF>
__global__ __launch_bounds__(256) void decode_kernel(const DecodeParams p) {
    constexpr int NT = 64 * WAVES, E = HmElem<DT>::per_chunk, ES = HmElem<DT>::size;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tid = WAVES == 1 ? lane : (int)threadIdx.x;            // index inside the team that shares the map
    const int m = WAVES == 1 ? (int)blockIdx.x * 4 + wave : (int)blockIdx.x;
    if (m >= p.total) return;                                        // whole waves (WAVES == 1) or nothing (WAVES == 4)
    const int j = m % p.J, v = (m / p.J) % p.V, b = m / (p.J * p.V);
    const int HW = p.H * p.W;
    const char* base = static_cast<const char*>(p.map(b, v, j, ES));
    const size_t bytes = (size_t)HW * ES;

    // what the finishing lane needs besides the map is fetched now, one value per lane, and handed over after the merge: the
    // latency of these loads hides under the scan and costs three registers there
    double cam = 0.0;
    float box = 0.0f;
    if (WAVES == 1 || wave == 0) {
        if (p.cams && lane < 16) cam = p.cams[v * 16 + lane];
        const size_t bv = ((size_t)b * p.V + v) * 2;
        if (p.center && lane < 3) box = lane < 2 ? p.center[bv + lane] : p.scale[bv];                // cx, cy, scale_x
    }

    float cur = -INFINITY;
    int idx = DECODE_EMPTY;
    float odd = 0.0f;
    const bool vec = ((reinterpret_cast<size_t>(base) | bytes) & 15) == 0;       // uniform over the team
    if (vec) {
        const int n16 = (int)(bytes >> 4), rounds = n16 / NT;                    // rounds in which every lane has a chunk
        const uint4* q = reinterpret_cast<const uint4*>(base) + tid;
        int rel = DECODE_EMPTY, k = 0;
        for (; k + 16 <= rounds; k += 16) hm_scan<DT, NT, 16>(q + (size_t)k * NT, k * NT * E, cur, rel, odd);
        if (k + 8 <= rounds) { hm_scan<DT, NT, 8>(q + (size_t)k * NT, k * NT * E, cur, rel, odd); k += 8; }
        if (k + 4 <= rounds) { hm_scan<DT, NT, 4>(q + (size_t)k * NT, k * NT * E, cur, rel, odd); k += 4; }
        for (; k * NT + tid < n16; ++k) hm_scan<DT, NT, 1>(q + (size_t)k * NT, k * NT * E, cur, rel, odd);
        if (rel != DECODE_EMPTY) idx = tid * E + rel;
    } else {
        for (int i = tid; i < HW; i += NT) {
            const float x = hm_load<DT>(base, i);
            if (x > cur) { cur = x; idx = i; }
            odd = fmaf(x, 0.0f, odd);
        }
    }
    if (odd != odd) {                                                // rare: the lane's first NaN, if it has one, over the elements it owns
        const int e_own = vec ? E : 1;
        bool found = false;
        for (int c = tid; !found && c * e_own < HW; c += NT)
            for (int e = 0; e < e_own; ++e) {
                const float x = hm_load<DT>(base, (size_t)c * e_own + e);
                if (x != x) { cur = x; idx = c * e_own + e; found = true; break; }
            }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(cur, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (hm_ahead(ov, oi, cur, idx)) { cur = ov; idx = oi; }
    }
    if (WAVES > 1) {
        __shared__ float sv[WAVES];
        __shared__ int si[WAVES];
        if (lane == 0) { sv[wave] = cur; si[wave] = idx; }
        __syncthreads();
        if (wave != 0) return;
        cur = sv[0]; idx = si[0];
#pragma unroll
        for (int k = 1; k < WAVES; ++k)
            if (hm_ahead(sv[k], si[k], cur, idx)) { cur = sv[k]; idx = si[k]; }
    }
    double c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = __shfl(cam, i, 64);
    const float box_x = __shfl(box, 0, 64), box_y = __shfl(box, 1, 64), box_s = __shfl(box, 2, 64);
    double rdx = 0.0, rdy = 0.0;                                     // the refinement's offset, where it applies
    if (RF == MPL_REFINE_CENTROID) {                                 // every lane holds the merged (cur, idx)
        if (cur > 0.0f && cur < INFINITY) hm_centroid<DT>(base, idx % p.W, idx / p.W, p.W, p.H, p.radius, p.threshold, lane, rdx, rdy);
    }
    if (lane != 0) return;

    if (idx == DECODE_EMPTY) idx = 0;                                // every value is -inf: np.argmax says 0
    const float maxval = cur;
    const bool positive = maxval > 0.0f;
    const int px = positive ? idx % p.W : 0, py = positive ? idx / p.W : 0;
    float cx = (float)px, cy = (float)py;
    if (RF == MPL_REFINE_NONE && p.post && 1 < px && px < p.W - 1 && 1 < py && py < p.H - 1) {
        const size_t at = (size_t)py * p.W + px;
        cx += hm_quarter(hm_load<DT>(base, at + 1), hm_load<DT>(base, at - 1));
        cy += hm_quarter(hm_load<DT>(base, at + p.W), hm_load<DT>(base, at - p.W));
    }
    if (RF != MPL_REFINE_NONE && positive && maxval < INFINITY) {
        if (RF == MPL_REFINE_GAUSSIAN) {
            const size_t at = (size_t)py * p.W + px;
            const double l0 = log((double)maxval);
            rdx = hm_log_quadratic<DT>(base, at, 1, px, p.W, l0);
            rdy = hm_log_quadratic<DT>(base, at, (size_t)p.W, py, p.H, l0);
        }
        cx = (float)((double)px + rdx);
        cy = (float)((double)py + rdy);
    }
    if (p.coords) {
        p.coords[(size_t)m * 2] = cx;
        p.coords[(size_t)m * 2 + 1] = cy;
    }
    double X = cx, Y = cy;
    if (p.center) {
        const double k = (double)box_s * 200.0 / (double)p.W;
        X = (double)box_x + (X - p.W * 0.5) * k;
        Y = (double)box_y + (Y - p.H * 0.5) * k;
    }
    const float fx = (float)X, fy = (float)Y;
    p.pixels[(size_t)m * 2] = fx;
    p.pixels[(size_t)m * 2 + 1] = fy;
    p.conf[m] = maxval;
    if (p.cams) {
        const size_t o = ((size_t)b * p.J + j) * 3;
        prepare_point(c, (double)fx, (double)fy, maxval, p.w, p.h, p.norm_in, p.norm_cam, p.out.poses[v] + o, p.out.rays[v] + o,
                      j == 0 ? p.out.centers[v] + (size_t)b * 3 : nullptr);
    }
}

template <int DT, int RF>
static void decode_launch(const DecodeParams& p, int waves, hipStream_t s) {
    if (waves == 4)
        hipLaunchKernelGGL((decode_kernel<DT, 4, RF>), dim3((unsigned)p.total), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((decode_kernel<DT, 1, RF>), dim3((unsigned)((p.total + 3) / 4)), dim3(256), 0, s, p);
}

template <int DT>
static void decode_launch(const DecodeParams& p, int waves, int refine, hipStream_t s) {
    if (refine == MPL_REFINE_GAUSSIAN) decode_launch<DT, MPL_REFINE_GAUSSIAN>(p, waves, s);
    else if (refine == MPL_REFINE_CENTROID) decode_launch<DT, MPL_REFINE_CENTROID>(p, waves, s);
    else decode_launch<DT, MPL_REFINE_NONE>(p, waves, s);
}

int launch_decode_heatmaps_ex(const void* const* heatmaps, int dtype, long long batch_stride, int B, int V, int J, int H, int W,
                              int post_process, const float* center, const float* scale, float* pixels, float* conf, float* coords,
                              const double* cams_dev, float img_w, float img_h, int norm_in, int norm_cam, float* const* poses,
                              float* const* rays, float* const* centers, int refine, int radius, double threshold, hipStream_t s) {
    if (!pixels || !conf || B <= 0 || V <= 0 || J <= 0 || H <= 0 || W <= 0) return MPL_E_INVALID;
    if ((center != nullptr) != (scale != nullptr)) return MPL_E_INVALID;
    if (cams_dev && (!poses || !rays || !centers || !(img_w > 0) || !(img_h > 0))) return MPL_E_INVALID;
    if (refine < MPL_REFINE_NONE || refine > MPL_REFINE_CENTROID || (refine != MPL_REFINE_NONE && post_process)) return MPL_E_INVALID;
    if (refine == MPL_REFINE_CENTROID && (radius < 1 || radius > 8 || threshold != threshold)) return MPL_E_INVALID;
    DecodeParams p;
    if (const int rc = heatmap_table_fill(p, heatmaps, dtype, batch_stride, B, V, J, H, W)) return rc;
    if ((long long)B * V * J > (1ll << 30)) return MPL_E_UNSUPPORTED;
    if (const int rc = view_outputs_fill(p.out, poses, rays, centers, V, cams_dev != nullptr)) return rc;
    p.center = center; p.scale = scale; p.cams = cams_dev; p.pixels = pixels; p.conf = conf; p.coords = coords;
    p.total = B * V * J; p.post = post_process;
    p.w = img_w; p.h = img_h; p.norm_in = norm_in; p.norm_cam = norm_cam;
    p.radius = refine == MPL_REFINE_CENTROID ? radius : 0; p.threshold = refine == MPL_REFINE_CENTROID ? threshold : 0.0;
    const int waves = decode_waves_per_map((size_t)H * W * (dtype == MPL_HM_F32 ? 4 : 2));
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dtype == MPL_HM_F32) decode_launch<MPL_HM_F32>(p, waves, refine, s);
    else if (dtype == MPL_HM_F16) decode_launch<MPL_HM_F16>(p, waves, refine, s);
    else decode_launch<MPL_HM_BF16>(p, waves, refine, s);
    return hip_check_launch();
}

int launch_decode_heatmaps(const void* const* heatmaps, int dtype, long long batch_stride, int B, int V, int J, int H, int W,
                           int post_process, const float* center, const float* scale, float* pixels, float* conf, float* coords,
                           const double* cams_dev, float img_w, float img_h, int norm_in, int norm_cam, float* const* poses,
                           float* const* rays, float* const* centers, hipStream_t s) {
    return launch_decode_heatmaps_ex(heatmaps, dtype, batch_stride, B, V, J, H, W, post_process, center, scale, pixels, conf, coords,
                                     cams_dev, img_w, img_h, norm_in, norm_cam, poses, rays, centers, MPL_REFINE_NONE, 0, 0.0, s);
}

}  // namespace mpl
