// Multi-view model inputs synthesized from 3D poses on the device: the producer in front of prepare_inputs_kernel, which the
// reference runs in numpy per sample and per view inside Dataset.__getitem__.
//
// Reference: pose placement MPL/lib/dataset/multiview_amass_h36m_mpl.py:317-342 (rotate_pose utils/utils_amass.py:3-34 about z,
// room translation); projection utils/calib.py:42-77 (cam_to_image(world_to_cam(X, R, -R t), K)); then
// lib/dataset/joints_dataset_mpl.py: detection noise and confidence penalty :592-613, visibility :701-727 (NO_AUGMENTATION),
// missing joints :735-740, normalisation / rays / centres :762-774, :615-623, :872-904 -- the arithmetic of inputs.hip, applied
// to the fp64 pixel.  One work item per (pose, view, joint), one launch, no LDS, no atomics, nothing depends on the launch
// geometry.  Arithmetic is fp64 on the fp32 tensors and every output is rounded once.
//
// Random numbers are the counter-based SplitMix64 draws of openmpl_amd/detrng.py (detrng.hpp): draw(key, i) = mix(key + (i + 1) * GOLD), top
// 53 bits -> [0,1).  The keys come from the host (detrng._stream_key); per-pose streams are indexed by first_index + b, per-joint
// streams by ((first_index + b) * V + v) * J + j, so a run cut into batches draws the values of the uncut run, and every (v, j)
// item of a pose recomputes the pose's rotation and translation from the same counter.
//
// The one deviation: a joint at z_cam <= 1e-9 (the reference divides anyway) gets confidence 0 and pixel (0,0) and skips the
// noise, visibility and missing-joint steps; its ray and normalised pose follow from that pixel.
//
// With a distortion table (mpl_synthesize_views_ex) step 2 projects through the lens model of views.hpp, steps 3 to 5 act on the
// distorted pixel, as a detector sees it, and step 6 is the arithmetic of mpl_prepare_inputs_ex: the ray goes through the
// undistorted pixel, a pixel that is not invertible keeps its pinhole ray and gets confidence 0.
#include "common.hpp"
#include "detrng.hpp"
#include "views.hpp"

namespace mpl {

struct SynthParams {                 // the pinhole launch: the kernel argument it has always had
    static constexpr bool DIST = false;
    ViewOutputs out;
    mpl_synth_options o;
    const float* x3d;        // (B,J,3)
    const double* cams;      // device (V,16) camera records
    const float* conf;       // (B,V,J) or null (-> 1)
    const float* rot_deg;    // (B) or null
    const float* trans;      // (B,3) or null
    const float* noise;      // (B,V,J,2) or null
    const float* miss_u;     // (B,V,J) or null
    float* target;           // (B,J,3) or null
    float* px;               // (B,V,J,2) or null: after step 5
    float* px_clean;         // (B,V,J,2) or null: after step 2
    float* depth;            // (B,V,J) or null: z_cam
    int has_views;           // poses / rays / centers are there
    int B, V, J;
};

struct SynthLensParams : SynthParams {
    static constexpr bool DIST = true;
    const double* dist;      // device (V,5) distortion records
};

// P::DIST: step 2 projects through the lens and step 6 sends the ray through the undistorted pixel (views.hpp).  The lens comes with
// its own argument type, so that the pinhole instantiation is the kernel it was, argument layout included
template <class P>
__global__ __launch_bounds__(256) void synthesize_views_kernel(const P p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)p.B * p.V * p.J;
    if (idx >= total) return;
    const int j = (int)(idx % p.J), v = (int)((idx / p.J) % p.V);
    const long long b = idx / ((long long)p.J * p.V);
    const mpl_synth_options& o = p.o;
    const unsigned long long gpose = (unsigned long long)(o.first_index + b);
    const unsigned long long gitem = (gpose * (unsigned long long)p.V + (unsigned long long)v) * (unsigned long long)p.J + (unsigned long long)j;

    // 1. pose placement: pose @ Rz^T about the origin, then + (tx, ty, 0)
    const float* xi = p.x3d + ((size_t)b * p.J + j) * 3;
    double X = xi[0], Y = xi[1], Z = xi[2];
    if (p.rot_deg || o.rotate) {
        const double deg = p.rot_deg ? (double)p.rot_deg[b] : detrng_draw(o.key_rot, gpose) * 360.0;
        const double a = deg * (3.141592653589793 / 180.0);
        const double ca = cos(a), sa = sin(a);
        const double x0 = X, y0 = Y;
        X = x0 * ca - y0 * sa;
        Y = x0 * sa + y0 * ca;
    }
    if (p.trans) {
        X += (double)p.trans[(size_t)b * 3];
        Y += (double)p.trans[(size_t)b * 3 + 1];
        Z += (double)p.trans[(size_t)b * 3 + 2];
    } else if (o.room) {
        X += detrng_draw(o.key_room_x, gpose) * (o.room_max_x - o.room_min_x) + o.room_min_x;
        Y += detrng_draw(o.key_room_y, gpose) * (o.room_max_y - o.room_min_y) + o.room_min_y;
    }

    // 2. projection: x_cam = R (X - t), px = (fx x / z + cx, fy y / z + cy)
    const double* c = p.cams + v * 16;
    const Camera cam{c};
    double xc, yc, zc;
    camera_coords(c, X, Y, Z, xc, yc, zc);
    const bool front = zc > CAMERA_Z_MIN;
    double x = 0.0, y = 0.0, cf = 0.0;
    if (front) {
        if constexpr (P::DIST) {       // px = fx (y0 g + p2 r2) + cx, the form of rpsm_project
            const Normalized yd = distort_normalized(xc / zc, yc / zc, distortion_of(p.dist, v));
            const Pixel px = pixel_of(cam, yd.x, yd.y);
            x = px.x;
            y = px.y;
        } else {                       // its own expression: fx * xc / zc rounds otherwise than fx * (xc / zc), and the pinhole goldens pin it
            x = cam.fx() * xc / zc + cam.cx();
            y = cam.fy() * yc / zc + cam.cy();
        }
        cf = p.conf ? (double)p.conf[idx] : 1.0;
    }
    if (p.px_clean) {
        p.px_clean[(size_t)idx * 2] = (float)x;
        p.px_clean[(size_t)idx * 2 + 1] = (float)y;
    }
    if (p.depth) p.depth[idx] = (float)zc;

    if (front) {
        // 3. detection noise and confidence penalty
        if (o.noise_level != 0.0) {
            double n0, n1;
            if (p.noise) {
                n0 = p.noise[(size_t)idx * 2];
                n1 = p.noise[(size_t)idx * 2 + 1];
            } else {   // Box-Muller
                const double u1 = 1.0 - detrng_draw(o.key_noise0, gitem), u2 = detrng_draw(o.key_noise1, gitem);
                const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
                n0 = r * cos(t);
                n1 = r * sin(t);
            }
            n0 *= o.noise_level;
            n1 *= o.noise_level;
            x += n0;
            y += n1;
            if (o.penalize != MPL_SYNTH_PENALIZE_NONE) {
                const double d = sqrt(n0 * n0 + n1 * n1);
                cf *= o.penalize == MPL_SYNTH_PENALIZE_EXP_ERROR ? o.penalize_a * exp(-o.penalize_b * d)
                      : o.penalize == MPL_SYNTH_PENALIZE_LINEAR ? o.penalize_a * d + o.penalize_b
                                                                  : exp(-d / 2.0);
            }
        }
        // 4. visibility
        const double w1 = o.img_w - 1.0, h1 = o.img_h - 1.0;
        if (o.clip) {
            if (!(0.0 < x && x < w1 && 0.0 < y && y < h1)) cf = 0.0;
            x = fmin(fmax(x, 0.0), w1);
            y = fmin(fmax(y, 0.0), h1);
        } else {
            if (cf > 0.0 && (fmin(x, y) < 0.0 || x >= o.img_w || y >= o.img_h)) cf = 0.0;
            if (!(cf > 0.0)) { x = 0.0; y = 0.0; }
        }
        // 5. missing joints
        if (o.missing_level > 0.0) {
            const double u = p.miss_u ? (double)p.miss_u[idx] : detrng_draw(o.key_missing, gitem);
            if (u < o.missing_level) { cf *= 0.0; x *= 0.0; y *= 0.0; }
        }
    }
    if (p.px) {
        p.px[(size_t)idx * 2] = (float)x;
        p.px[(size_t)idx * 2 + 1] = (float)y;
    }

    // 6. normalisation, rays, centres: prepare_inputs_kernel on the fp64 pixel.  The compiler barrier makes prepare_point read the
    // camera record again, as step 6 always has: held in registers across steps 3 to 5, R and t cost 24 VGPRs and two occupancy steps
    if (p.has_views) {
        asm volatile("" ::: "memory");
        const size_t ob = ((size_t)b * p.J + j) * 3;
        if constexpr (P::DIST)
            prepare_point_undistorted(c, distortion_of(p.dist, v), x, y, (float)cf, o.img_w, o.img_h, o.normalize_inputs,
                                      o.normalize_cameras, p.out.poses[v] + ob, p.out.rays[v] + ob,
                                      j == 0 ? p.out.centers[v] + (size_t)b * 3 : nullptr);
        else
            prepare_point(c, x, y, (float)cf, o.img_w, o.img_h, o.normalize_inputs, o.normalize_cameras, p.out.poses[v] + ob,
                          p.out.rays[v] + ob, j == 0 ? p.out.centers[v] + (size_t)b * 3 : nullptr);
    }

    // 7. target
    if (p.target && v == 0) {
        float* to = p.target + ((size_t)b * p.J + j) * 3;
        to[0] = (float)((X - o.target_offset[0]) / o.target_scale[0]);
        to[1] = (float)((Y - o.target_offset[1]) / o.target_scale[1]);
        to[2] = (float)((Z - o.target_offset[2]) / o.target_scale[2]);
    }
}

int launch_synthesize_views(const float* poses3d, const double* cams_dev, const double* dist_dev, const mpl_synth_options* opt, const float* conf,
                            const float* rotation_deg, const float* translation, const float* noise, const float* missing_u,
                            int B, int V, int J, float* const* poses, float* const* rays, float* const* centers, float* target,
                            float* pixels, float* pixels_clean, float* depth, hipStream_t s) {
    if (!poses3d || !cams_dev || !opt || B <= 0 || V <= 0 || V > MPL_MAX_VIEWS || J <= 0) return MPL_E_INVALID;
    if (!(opt->img_w > 0.0) || !(opt->img_h > 0.0)) return MPL_E_INVALID;
    if (opt->penalize < MPL_SYNTH_PENALIZE_NONE || opt->penalize > MPL_SYNTH_PENALIZE_EXP_SQRT) return MPL_E_INVALID;
    for (int d = 0; d < 3; ++d)
        if (opt->target_scale[d] == 0.0 || opt->target_scale[d] != opt->target_scale[d]) return MPL_E_INVALID;
    const bool any = poses || rays || centers;
    if (any && (!poses || !rays || !centers)) return MPL_E_INVALID;
    if (!any && !target && !pixels && !pixels_clean && !depth) return MPL_E_INVALID;
    const long long total = (long long)B * V * J;
    if (total > (1ll << 36)) return MPL_E_UNSUPPORTED;
    SynthLensParams p;
    if (const int rc = view_outputs_fill(p.out, poses, rays, centers, V, any)) return rc;
    p.o = *opt;
    p.x3d = poses3d; p.cams = cams_dev; p.conf = conf; p.rot_deg = rotation_deg; p.trans = translation; p.noise = noise;
    p.miss_u = missing_u; p.target = target; p.px = pixels; p.px_clean = pixels_clean; p.depth = depth;
    p.has_views = any; p.B = B; p.V = V; p.J = J; p.dist = dist_dev;
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    if (dist_dev)
        hipLaunchKernelGGL(synthesize_views_kernel<SynthLensParams>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL(synthesize_views_kernel<SynthParams>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                           static_cast<const SynthParams&>(p));
    return hip_check_launch();
}

}  // namespace mpl
