// Heatmaps rendered from 2D joints on the device: the producer in front of decode_kernel and the rpsm kernels, which the reference
// runs in numpy per joint inside Dataset.__getitem__ (the target maker of its 2D stage).
//
// Reference (MPL/lib/dataset/joints_dataset_mpl.py:828-870 generate_heatmap): mu = int(joint / feat_stride + 0.5), a patch of
// mu +/- 3 sigma holding exp(-(dx^2 + dy^2) / (2 sigma^2)) at integer dx, dy, zero elsewhere; target_weight = the joint's
// visibility, 0 when the patch lies wholly outside the map, and the patch is written only where the weight is above 0.5.  That
// is MPL_RENDER_REFERENCE.  MPL_RENDER_SUBPIXEL is conf * exp(-((x - mx)^2 + (y - my)^2) / (2 sigma^2)) on every cell about the
// real-valued cell (mx, my), what a detector's map looks like.  The one deviation: a cell that is not finite or beyond +/-2^30
// gives a zero map and weight 0 (the reference's int(nan) raises).
//
// One launch, one wave per map, four maps per 256-thread workgroup (the shape of decode_kernel).  The Gaussian is separable:
// value(x, y) = gx(x) * gy(y) with gx(x) = exp(-(x - cx)^2 / (2 sigma^2)) and gy(y) = amp * exp(-(y - cy)^2 / (2 sigma^2)), all
// fp64, the product rounded once to the map's dtype (hm_narrow).  For a map of at most 64 x 64 cells lane l computes gx(l) and
// gy(l) -- W + H exponentials per map -- and every cell is two lane reads and one multiply; a larger map evaluates both factors
// per cell.  Both give the same bits, because a factor depends on its coordinate only.  A map whose base address and byte size
// are multiples of 16 is written with 16-byte stores, any other element by element.  No atomics, no scratch, no LDS.
//
// Noise: noise_level * u is added to every cell before the rounding, u = draw (global map index) * H * W + y * W + x of the
// stream `noise_key` (detrng.hpp), the global map index being ((first_index + b) * V + v) * J + j: a run cut into batches is the
// uncut run.
#include "common.hpp"
#include "detrng.hpp"
#include "views.hpp"

namespace mpl {

struct RenderParams : HeatmapTable {
    const float* pixels;             // (B,V,J,2)
    const float* conf;               // (B,V,J) or null (-> 1)
    const float* center;             // (B,V,2) or null
    const float* scale;              // (B,V,2) or null; component 1 is not read
    float* weight;                   // (B,V,J)
    float* cells;                    // (B,V,J,2)
    double stride_x, stride_y;       // 0: no stride
    double two_s2;                   // 2 sigma^2
    double reach;                    // reference mode: 3 sigma, an integer; sub-pixel mode: +inf
    double noise;                    // 0: none drawn
    unsigned long long key, first_index;
    int total, mode;
};

constexpr double RENDER_CELL_MAX = 1073741824.0;     // 2^30

// one factor of the separable Gaussian at integer coordinate c about centre m; outside the reach it is 0
__device__ __forceinline__ double render_factor(int c, double m, double reach, double two_s2) {
    const double d = (double)c - m;
    return fabs(d) > reach ? 0.0 : exp(-(d * d) / two_s2);
}

__device__ __forceinline__ double render_shfl(double x, int src) { return __shfl(x, src, 64); }

template <int DT>
__global__ __launch_bounds__(256) void render_kernel(const RenderParams p) {
    constexpr int ES = DT == MPL_HM_F32 ? 4 : 2, E = 16 / ES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = (int)blockIdx.x * 4 + wave;
    if (m >= p.total) return;                                        // whole waves
    const int j = m % p.J, v = (m / p.J) % p.V, b = m / (p.J * p.V);
    const int W = p.W, H = p.H, HW = H * W;
    char* base = const_cast<char*>(static_cast<const char*>(p.map(b, v, j, ES)));
    const size_t bytes = (size_t)HW * ES;

    // the joint's cell, the same in every lane
    double mx = p.pixels[(size_t)m * 2], my = p.pixels[(size_t)m * 2 + 1];
    if (p.center) {
        const size_t bv = ((size_t)b * p.V + v) * 2;
        const double k = (double)p.scale[bv] * 200.0 / (double)W;
        mx = (mx - (double)p.center[bv]) / k + W * 0.5;
        my = (my - (double)p.center[bv + 1]) / k + H * 0.5;
    } else if (p.stride_x != 0.0) {
        mx = mx / p.stride_x;
        my = my / p.stride_y;
    }
    const float cf = p.conf ? p.conf[m] : 1.0f;
    const bool finite = fabs(mx) <= RENDER_CELL_MAX && fabs(my) <= RENDER_CELL_MAX;      // false for NaN
    double cx = mx, cy = my, amp = 1.0;
    float wt;
    bool on;
    if (p.mode == MPL_RENDER_REFERENCE) {
        cx = trunc(mx + 0.5);                                        // Python's int(): towards zero
        cy = trunc(my + 0.5);
        const bool outside = cx - p.reach >= W || cy - p.reach >= H || cx + p.reach + 1.0 < 0.0 || cy + p.reach + 1.0 < 0.0;
        wt = finite && !outside ? cf : 0.0f;
        on = wt > 0.5f;
    } else {
        on = finite && cf > 0.0f;
        wt = on ? cf : 0.0f;
        amp = cf;
    }
    if (lane == 0) {
        p.weight[m] = wt;
        p.cells[(size_t)m * 2] = (float)mx;
        p.cells[(size_t)m * 2 + 1] = (float)my;
    }

    const bool small = W <= 64 && H <= 64;                           // the factors live in the lanes
    double gxl = 0.0, gyl = 0.0;
    if (small && on) {
        if (lane < W) gxl = render_factor(lane, cx, p.reach, p.two_s2);
        if (lane < H) gyl = amp * render_factor(lane, cy, p.reach, p.two_s2);
    }
    const unsigned long long first = (((p.first_index + (unsigned long long)b) * (unsigned long long)p.V + (unsigned long long)v) *
                                          (unsigned long long)p.J + (unsigned long long)j) * (unsigned long long)HW;
    // the fp64 value of cell (x, y), i its index in the map; called by all lanes of the wave together
    auto cell = [&](double fx, double fy, int i) {
        double val = fx * fy;
        if (p.noise != 0.0) val += p.noise * detrng_draw(p.key, first + (unsigned long long)i);
        return val;
    };
    auto factor_x = [&](int x) { return small ? render_shfl(gxl, x) : (on ? render_factor(x, cx, p.reach, p.two_s2) : 0.0); };
    auto factor_y = [&](int y) { return small ? render_shfl(gyl, y) : (on ? amp * render_factor(y, cy, p.reach, p.two_s2) : 0.0); };

    if (((reinterpret_cast<size_t>(base) | bytes) & 15) == 0) {
        const int n16 = (int)(bytes >> 4), rounds = (n16 + 63) >> 6;     // the same trip count in every lane: the lane reads need all
        const bool one_row = W % E == 0;                             // a chunk does not straddle two rows
        // a chunk lies in one row and a round of 64 chunks is a whole number of rows: a lane keeps its E columns, and its row
        // advances by the same step.  Without one_row (W < E among them) every element finds its own row and column
        const bool fixed = small && one_row && (64 * E) % W == 0;
        double fxe[E];
        int y0 = 0, step = 0;
        if (fixed) {
#pragma unroll
            for (int e = 0; e < E; ++e) fxe[e] = render_shfl(gxl, (lane * E + e) % W);
            y0 = lane * E / W;
            step = 64 * E / W;
        }
        uint4* q = reinterpret_cast<uint4*>(base);
        for (int k = 0; k < rounds; ++k) {
            const int c = k * 64 + lane, i0 = c * E;
            unsigned bits[E];
            double fy = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = i0 + e;
                if (e == 0 || !one_row) fy = factor_y(min(fixed ? y0 + k * step : i / W, H - 1));
                const double fx = fixed ? fxe[e] : factor_x(i % W);
                bits[e] = hm_narrow<DT>(cell(fx, fy, i));
            }
            uint4 o;
            if (DT == MPL_HM_F32) {
                o = make_uint4(bits[0], bits[1], bits[2], bits[3]);
            } else {
                o = make_uint4(bits[0] | bits[1 % E] << 16, bits[2 % E] | bits[3 % E] << 16, bits[4 % E] | bits[5 % E] << 16,
                               bits[6 % E] | bits[7 % E] << 16);
            }
            if (c < n16) q[c] = o;
        }
    } else {
        const int rounds = (HW + 63) >> 6;
        for (int k = 0; k < rounds; ++k) {
            const int i = k * 64 + lane;
            const double fy = factor_y(min(i / W, H - 1));
            const double fx = factor_x(i % W);
            const unsigned bits = hm_narrow<DT>(cell(fx, fy, i));
            if (i < HW) {
                if (DT == MPL_HM_F32) reinterpret_cast<unsigned*>(base)[i] = bits;
                else reinterpret_cast<unsigned short*>(base)[i] = (unsigned short)bits;
            }
        }
    }
}

int launch_render_heatmaps(void* const* heatmaps, int dtype, long long batch_stride, int B, int V, int J, int H, int W,
                           const float* pixels, const float* conf, const float* center, const float* scale, double stride_x,
                           double stride_y, int mode, double sigma, double noise_level, unsigned long long noise_key,
                           long long first_index, float* weight, float* cells, hipStream_t s) {
    if (!pixels || !weight || !cells || B <= 0 || V <= 0 || J <= 0 || H <= 0 || W <= 0) return MPL_E_INVALID;
    if ((center != nullptr) != (scale != nullptr)) return MPL_E_INVALID;
    if ((stride_x != 0.0) != (stride_y != 0.0) || !(stride_x >= 0.0) || !(stride_y >= 0.0) || stride_x > 1e300 || stride_y > 1e300)
        return MPL_E_INVALID;
    if (center && stride_x != 0.0) return MPL_E_INVALID;
    if (mode != MPL_RENDER_REFERENCE && mode != MPL_RENDER_SUBPIXEL) return MPL_E_INVALID;
    if (!(sigma > 0.0) || sigma > 1e6 || !(noise_level >= 0.0) || noise_level > 1e300 || first_index < 0) return MPL_E_INVALID;
    if (mode == MPL_RENDER_REFERENCE && 3.0 * sigma != floor(3.0 * sigma)) return MPL_E_INVALID;
    RenderParams p;
    if (const int rc = heatmap_table_fill(p, heatmaps, dtype, batch_stride, B, V, J, H, W)) return rc;
    if ((long long)B * V * J > (1ll << 30)) return MPL_E_UNSUPPORTED;
    p.pixels = pixels; p.conf = conf; p.center = center; p.scale = scale; p.weight = weight; p.cells = cells;
    p.stride_x = stride_x; p.stride_y = stride_y;
    p.two_s2 = 2.0 * sigma * sigma;
    p.reach = mode == MPL_RENDER_REFERENCE ? 3.0 * sigma : INFINITY;
    p.noise = noise_level; p.key = noise_key; p.first_index = (unsigned long long)first_index;
    p.total = B * V * J; p.mode = mode;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    const dim3 grid((unsigned)((p.total + 3) / 4));
    if (dtype == MPL_HM_F32) hipLaunchKernelGGL(render_kernel<MPL_HM_F32>, grid, dim3(256), 0, s, p);
    else if (dtype == MPL_HM_F16) hipLaunchKernelGGL(render_kernel<MPL_HM_F16>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(render_kernel<MPL_HM_BF16>, grid, dim3(256), 0, s, p);
    return hip_check_launch();
}

}  // namespace mpl
