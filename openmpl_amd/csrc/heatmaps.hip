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

template <int DT, int WAVES>
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
    if (lane != 0) return;

    if (idx == DECODE_EMPTY) idx = 0;                                // every value is -inf: np.argmax says 0
    const float maxval = cur;
    const bool positive = maxval > 0.0f;
    const int px = positive ? idx % p.W : 0, py = positive ? idx / p.W : 0;
    float cx = (float)px, cy = (float)py;
    if (p.post && 1 < px && px < p.W - 1 && 1 < py && py < p.H - 1) {
        const size_t at = (size_t)py * p.W + px;
        cx += hm_quarter(hm_load<DT>(base, at + 1), hm_load<DT>(base, at - 1));
        cy += hm_quarter(hm_load<DT>(base, at + p.W), hm_load<DT>(base, at - p.W));
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

template <int DT>
static void decode_launch(const DecodeParams& p, int waves, hipStream_t s) {
    if (waves == 4)
        hipLaunchKernelGGL((decode_kernel<DT, 4>), dim3((unsigned)p.total), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((decode_kernel<DT, 1>), dim3((unsigned)((p.total + 3) / 4)), dim3(256), 0, s, p);
}

int launch_decode_heatmaps(const void* const* heatmaps, int dtype, long long batch_stride, int B, int V, int J, int H, int W,
                           int post_process, const float* center, const float* scale, float* pixels, float* conf, float* coords,
                           const double* cams_dev, float img_w, float img_h, int norm_in, int norm_cam, float* const* poses,
                           float* const* rays, float* const* centers, hipStream_t s) {
    if (!pixels || !conf || B <= 0 || V <= 0 || J <= 0 || H <= 0 || W <= 0) return MPL_E_INVALID;
    if ((center != nullptr) != (scale != nullptr)) return MPL_E_INVALID;
    if (cams_dev && (!poses || !rays || !centers || !(img_w > 0) || !(img_h > 0))) return MPL_E_INVALID;
    DecodeParams p;
    if (const int rc = heatmap_table_fill(p, heatmaps, dtype, batch_stride, B, V, J, H, W)) return rc;
    if ((long long)B * V * J > (1ll << 30)) return MPL_E_UNSUPPORTED;
    if (const int rc = view_outputs_fill(p.out, poses, rays, centers, V, cams_dev != nullptr)) return rc;
    p.center = center; p.scale = scale; p.cams = cams_dev; p.pixels = pixels; p.conf = conf; p.coords = coords;
    p.total = B * V * J; p.post = post_process;
    p.w = img_w; p.h = img_h; p.norm_in = norm_in; p.norm_cam = norm_cam;
    const int waves = decode_waves_per_map((size_t)H * W * (dtype == MPL_HM_F32 ? 4 : 2));
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dtype == MPL_HM_F32) decode_launch<MPL_HM_F32>(p, waves, s);
    else if (dtype == MPL_HM_F16) decode_launch<MPL_HM_F16>(p, waves, s);
    else decode_launch<MPL_HM_BF16>(p, waves, s);
    return hip_check_launch();
}

}  // namespace mpl
