// Host-side exerciser of libmpl_hip.so for the ASan + UBSan job (tests/test_sanitize_cpu.py; SURVEY.md section 5 "sanitizers").
// The library is built HOST-ONLY for it (hipcc --cuda-host-only -fsanitize=address,undefined: no device code objects, GPU
// sanitizers are not available on this pool) and this program walks what the host side of csrc/api.hip does WITHOUT a GPU:
// argument validation, workspace carving arithmetic, the schedule arrays, struct marshalling, the error strings and the
// per-device state (mutex / event chain, error word, profile brackets), and the caller's host arrays that the geometry, heatmap,
// track and evaluator entry points read before they launch (walk() and the walk_* functions, called at the end of main).  Every entry point that needs a
// device must come back with an MPL_E_* code -- never a crash, a leak, an out-of-bounds access or undefined behaviour.
// Test infrastructure: nothing under openmpl_amd/ uses it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "mpl_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "EXPECT failed at line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------------------------
// The walk of one entry point whose host side reads caller arrays before it launches (segments, pairs, keys, the per-view pointer
// lists, parents, the option structs) and multiplies sizes in int.  An entry point is written once, as a lambda that makes the
// well-formed call: every pointer argument goes through P(i, .) and every size through S(i, .), and walk() repeats the call
// with each pointer NULL in turn and each size at 0, negative, its documented limit, its limit + 1 and at values whose int
// products overflow.  The lambda allocates every HOST array on the heap at exactly the length the call documents for the sizes
// of that repetition (std::vector: one allocation of that many elements), so a read behind one is an ASan report.  Without a
// device every repetition answers with a negative code, a required pointer at NULL and an optional one alike: the negative code
// is only the least a call must do, and the check of these repetitions is the sanitizers' (a NULL that is dereferenced, a host
// array read behind its end, an int product that overflows).  tests/test_sanitize_cpu.py holds the set of declared entry points
// against the names in this file.
static int g_null = -1, g_size = -1;
static long long g_value = 0;
static const char* g_name = "";
template <class T>
static T* P(int i, T* p) { return i == g_null ? nullptr : p; }
static int S(int i, long long v) { return (int)(i == g_size ? g_value : v); }
static long long SL(int i, long long v) { return i == g_size ? g_value : v; }
// the length of a host array that the call documents as n entries, n at most `limit`: a refused n reads nothing
// the workspace of a call goes through WS(pointer) and WSB(bytes): walk() repeats the call with it one byte short and misaligned
static int g_ws = 0;
static bool g_ws_used = false;
static void* WS(void* p) { g_ws_used = true; return g_ws == 2 && p ? (void*)((char*)p + 1) : p; }
static size_t WSB(size_t bytes) { return g_ws == 1 && bytes ? bytes - 1 : bytes; }
static size_t len(long long n, long long limit = 128) { return (size_t)(n < 0 ? 0 : n > limit + 1 ? limit + 1 : n); }

struct Size { int index; long long limit; };      // limit 0: none documented for the argument alone

static void negative(int rc, const char* what, long long v) {
    if (rc >= 0) {
        std::fprintf(stderr, "%s: %s %lld answered %d, not a negative code\n", g_name, what, v, rc);
        ++failures;
    }
}

template <class F>
static void walk(const char* name, int n_ptrs, std::initializer_list<Size> sizes, F call) {
    g_name = name;
    g_null = g_size = -1;
    g_ws = 0;
    g_ws_used = false;
    negative(call(), "the well-formed call", 0);
    for (g_ws = 1; g_ws_used && g_ws <= 2; ++g_ws) negative(call(), g_ws == 1 ? "a workspace one byte short, case" : "a misaligned workspace, case", g_ws);
    g_ws = 0;
    for (g_null = 0; g_null < n_ptrs; ++g_null) negative(call(), "NULL for pointer", g_null);
    g_null = -1;
    for (const Size& s : sizes) {
        g_size = s.index;
        for (long long v : {0ll, -1ll, -2147483647ll - 1, 65536ll, 2147483647ll}) {
            g_value = v;
            negative(call(), "a size of", v);
        }
        for (long long v : {s.limit, s.limit + 1}) {
            if (s.limit == 0) break;
            g_value = v;
            negative(call(), "a size of", v);
        }
    }
    g_size = -1;
}

static std::vector<float> g_fake(4096, 0.f);       // stands in for every device tensor: opaque to the host side
template <class T>
static T* dev() { return reinterpret_cast<T*>(g_fake.data()); }

static void walk_queries() {
    for (int dim : {-1, 0, 7, 32, 136, 544, 1088, 4096, 4097, 65536, 2147483647})
        for (int heads : {-1, 0, 1, 3, 8, 16, 2147483647})
            for (int n_tok : {-1, 0, 1, 2, 31, 32, 33, 2048, 65536, 2147483647}) {
                (void)mpl_bf16_operand_layout(dim, heads, n_tok);
                (void)mpl_team_stack_shape(dim, heads, n_tok);
            }
    EXPECT(mpl_config_supported(nullptr) < 0);
    for (int J : {-1, 0, 1, 17, 64, 65, 65536, 2147483647})
        for (int d : {-1, 0, 1, 24, 32, 128, 129, 65536, 2147483647})
            for (int H : {-1, 0, 1, 2, 8, 2147483647})
                for (int V : {-1, 0, 1, MPL_MAX_VIEWS, MPL_MAX_VIEWS + 1, 2147483647})
                    for (unsigned f : {0u, (unsigned)MPL_F_POS3D_LEARN, (unsigned)(MPL_F_KPTOK | MPL_F_POS3D_LEARN), (unsigned)MPL_F_RAYS_TOKEN, ~0u}) {
                        mpl_config c{J, d, 2, H, V, 2, f, 0};
                        const int rc = mpl_config_supported(&c);
                        EXPECT(rc <= 0);
                        if (J <= 0 || d <= 0 || H <= 0 || V <= 0 || J > 64 || d > 128 || V > MPL_MAX_VIEWS) EXPECT(rc < 0);
                    }
    for (int B : {-1, 0, 1, 1 << 20, (1 << 20) + 1, 2147483647})
        for (int J : {-1, 0, 1, 64, 65, 2147483647})
            for (int n : {-1, 0, 1, 2, 16, 17, 65536, 2147483647}) {
                const size_t b = mpl_rpsm_workspace_bytes(B, J, n);
                if (B <= 0 || J <= 0 || J > 64 || n < 2 || n > 16 || B > (1 << 20)) EXPECT(b == 0);
            }
    for (int B : {-1, 0, 1, 1 << 15, 1 << 24, 2147483647})
        for (int V : {-1, 0, 1, MPL_MAX_VIEWS, MPL_MAX_VIEWS + 1, 65536, 2147483647})
            for (int J : {-1, 0, 1, 64, 65, 65536, 2147483647}) {
                const size_t a = mpl_locate_cameras_workspace_bytes(B, V, J), b = mpl_relative_pose_workspace_bytes(B, V, J);
                const bool outside = B <= 0 || V <= 0 || J <= 0 || V > MPL_MAX_VIEWS || J > 64 || (long long)B * V * J > (1ll << 30);
                if (outside) EXPECT(a == 0 && b == 0);
            }
    for (long long T : {-1ll, 0ll, 1ll, 33ll, (long long)MPL_SMOOTH_MAX_FRAMES, (long long)MPL_SMOOTH_MAX_FRAMES + 1, 1ll << 31, 1ll << 62})
        for (int J : {-1, 0, 1, MPL_SMOOTH_MAX_JOINTS, MPL_SMOOTH_MAX_JOINTS + 1, 2147483647})
            for (int n : {-1, 0, 1, 256, 65536, 2147483647}) {
                const size_t b = mpl_smooth_tracks_workspace_bytes(T, J, n);
                if (T < 1 || T > MPL_SMOOTH_MAX_FRAMES || J < 1 || J > MPL_SMOOTH_MAX_JOINTS || n < 1 || n > T) EXPECT(b == 0);
                else EXPECT(b >= (size_t)T * J * MPL_SMOOTH_WS_DOUBLES * sizeof(double));
            }
    for (int a : {-1, 0, 1, 17, 64, 65, 65536, 2147483647})
        for (int g : {-1, 0, 1, MPL_EVAL_MAX_GROUPS, MPL_EVAL_MAX_GROUPS + 1, 65536, 2147483647}) {
            const size_t b = mpl_eval_state_bytes(a, g);
            const int r = mpl_eval_report_size(a, g);
            if (a <= 0 || a > 64 || g <= 0 || g > MPL_EVAL_MAX_GROUPS) EXPECT(b == 0 && r <= 0);
            else EXPECT(b > 0 && r == 8 + 2 * g * (4 * a + 5));
        }
    for (int a : {-1, 0, 1, 51, 96, 544, 4096, 4097, 65536, 2147483647})
        for (int b : {-1, 0, 1, 31, 32, 100, 480, 4096, 4097, 65536, 2147483647}) {
            (void)mpl_pack_bf16_any_bytes(a, b);
            (void)mpl_ln_linear_bf16_any_workspace_bytes(a, b);
        }
}

static void walk_heatmaps() {
    for (int ex = 0; ex < 4; ++ex) {
        auto call = [&]() {
            const int B = S(0, 2), V = S(1, 3), J = S(2, 17), H = S(3, 64), W = S(4, 48);
            std::vector<const void*> maps(len(V), dev<void>());
            std::vector<float*> lists(len(V), dev<float>());
            const long long stride = (long long)J * H * W;
            if (ex == 0)
                return mpl_decode_heatmaps(P(0, maps.data()), MPL_HM_F16, stride, B, V, J, H, W, 1, P(1, dev<float>()), P(2, dev<float>()),
                                           P(3, dev<float>()), P(4, dev<float>()), P(5, dev<float>()), P(6, dev<double>()), 1000.f, 1000.f, 1, 1,
                                           P(7, lists.data()), P(8, lists.data()), P(9, lists.data()), nullptr);
            return mpl_decode_heatmaps_ex(P(0, maps.data()), ex == 3 ? 7 : MPL_HM_F32, stride, B, V, J, H, W, 0, P(1, dev<float>()), P(2, dev<float>()),
                                          P(3, dev<float>()), P(4, dev<float>()), P(5, dev<float>()), P(6, dev<double>()), 1000.f, 1000.f, 1, 1,
                                          P(7, lists.data()), P(8, lists.data()), P(9, lists.data()), ex == 1 ? MPL_REFINE_GAUSSIAN : MPL_REFINE_CENTROID,
                                          ex == 1 ? 0 : 8, 0.1, nullptr);
        };
        walk(ex ? "mpl_decode_heatmaps_ex" : "mpl_decode_heatmaps", 10, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 0}, {3, 0}, {4, 0}}, call);
    }
    {
        std::vector<const void*> maps(3, dev<void>());
        std::vector<float*> lists(3, dev<float>());
        maps[2] = nullptr;          // a NULL entry among the first `views`
        EXPECT(mpl_decode_heatmaps(maps.data(), MPL_HM_F32, 17 * 64 * 64, 2, 3, 17, 64, 64, 0, nullptr, nullptr, dev<float>(), dev<float>(), nullptr,
                                   nullptr, 0.f, 0.f, 0, 0, nullptr, nullptr, nullptr, nullptr) < 0);
        maps[2] = dev<void>();
        lists[1] = nullptr;
        EXPECT(mpl_decode_heatmaps(maps.data(), MPL_HM_F32, 17 * 64 * 64, 2, 3, 17, 64, 64, 0, nullptr, nullptr, dev<float>(), dev<float>(), nullptr,
                                   dev<double>(), 1000.f, 1000.f, 0, 0, lists.data(), lists.data(), lists.data(), nullptr) < 0);
        EXPECT(mpl_decode_heatmaps(maps.data(), MPL_HM_F32, 17 * 64 * 64 - 1, 2, 3, 17, 64, 64, 0, nullptr, nullptr, dev<float>(), dev<float>(), nullptr,
                                   nullptr, 0.f, 0.f, 0, 0, nullptr, nullptr, nullptr, nullptr) < 0);
        EXPECT(mpl_decode_heatmaps(maps.data(), MPL_HM_F32, 1ll << 40, 1 << 20, 3, 17, 1024, 1025, 0, nullptr, nullptr, dev<float>(), dev<float>(), nullptr,
                                   nullptr, 0.f, 0.f, 0, 0, nullptr, nullptr, nullptr, nullptr) < 0);
        for (int radius : {-1, 0, 9}) EXPECT(mpl_decode_heatmaps_ex(maps.data(), MPL_HM_F32, 17 * 64 * 64, 2, 3, 17, 64, 64, 0, nullptr, nullptr, dev<float>(), dev<float>(), nullptr,
                                                                   nullptr, 0.f, 0.f, 0, 0, nullptr, nullptr, nullptr, MPL_REFINE_CENTROID, radius, 0.0, nullptr) < 0);
    }
    for (int mode : {MPL_RENDER_REFERENCE, MPL_RENDER_SUBPIXEL, 5}) {
        auto call = [&]() {
            const int B = S(0, 2), V = S(1, 3), J = S(2, 17), H = S(3, 64), W = S(4, 48);
            std::vector<void*> maps(len(V), dev<void>());
            return mpl_render_heatmaps(P(0, maps.data()), MPL_HM_BF16, (long long)J * H * W, B, V, J, H, W, P(1, dev<float>()), P(2, dev<float>()),
                                       P(3, dev<float>()), P(4, dev<float>()), 0.0, 0.0, mode, 2.0, 0.01, 77u, SL(5, 1000003), P(5, dev<float>()),
                                       P(6, dev<float>()), nullptr);
        };
        walk("mpl_render_heatmaps", 7, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 0}, {3, 0}, {4, 0}}, call);
    }
    {
        auto call = [&]() {
            const int B = S(0, 2), V = S(1, 3), J = S(2, 17), H = S(3, 64), W = S(4, 48), n0 = S(5, 16), n1 = S(6, 2), depth = S(7, 3);
            std::vector<const void*> maps(len(V), dev<void>());
            std::vector<int> parents(len(J, 64));
            for (size_t j = 0; j < parents.size(); ++j) parents[j] = (int)j - 1;
            const size_t wsb = mpl_rpsm_workspace_bytes(B, J, n0);
            return mpl_rpsm(P(0, maps.data()), MPL_HM_F32, (long long)J * H * W, B, V, J, H, W, P(1, dev<float>()), P(2, dev<float>()), P(3, dev<double>()),
                            P(4, dev<double>()), 1000.0, 1000.0, P(5, dev<float>()), P(6, dev<float>()), SL(8, J), P(7, parents.data()), n0, n1, depth, 2000.0,
                            150.0, P(8, WS(dev<void>())), WSB(wsb), P(9, dev<float>()), P(10, dev<int32_t>()), P(11, dev<double>()), MPL_RPSM_ALL, nullptr);
        };
        walk("mpl_rpsm", 12, {{0, 1 << 20}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 0}, {4, 0}, {5, 16}, {6, 4}, {7, 16}}, call);
        std::vector<const void*> maps(3, dev<void>());
        const size_t wsb = mpl_rpsm_workspace_bytes(2, 17, 16);
        EXPECT(wsb > 0);
        for (int kind = 0; kind < 8; ++kind) {
            std::vector<int> parents(17);
            for (int j = 0; j < 17; ++j) parents[j] = j - 1;
            if (kind == 0) parents[5] = -1;               // two roots
            if (kind == 1) parents[0] = 3;                // no root
            if (kind == 2) parents[7] = 17;               // a parent that is no joint
            if (kind == 3) parents[7] = 7;                // its own parent
            if (kind == 4) parents[3] = 9, parents[9] = 3;
            const size_t bytes = kind == 5 ? wsb - 1 : kind == 7 ? 0 : wsb;
            void* ws = kind == 6 ? (void*)((char*)g_fake.data() + 1) : dev<void>();          // misaligned
            EXPECT(mpl_rpsm(maps.data(), MPL_HM_F32, 17 * 64 * 64, 2, 3, 17, 64, 64, dev<float>(), dev<float>(), dev<double>(), nullptr, 1000.0, 1000.0,
                            dev<float>(), dev<float>(), 0, parents.data(), 16, 2, 3, 2000.0, 150.0, ws, bytes, dev<float>(), dev<int32_t>(),
                            dev<double>(), MPL_RPSM_ALL, nullptr) < 0);
        }
        std::vector<int> parents(17);
        for (int j = 0; j < 17; ++j) parents[j] = j - 1;
        for (int stages : {0, 8, -1})
            EXPECT(mpl_rpsm(maps.data(), MPL_HM_F32, 17 * 64 * 64, 2, 3, 17, 64, 64, dev<float>(), dev<float>(), dev<double>(), nullptr, 1000.0, 1000.0,
                            dev<float>(), dev<float>(), 0, parents.data(), 16, 2, 3, 2000.0, 150.0, dev<void>(), wsb, dev<float>(), dev<int32_t>(),
                            dev<double>(), stages, nullptr) < 0);
        EXPECT(mpl_rpsm(maps.data(), MPL_HM_F32, 17 * 64 * 64, 2, 3, 17, 64, 64, dev<float>(), dev<float>(), dev<double>(), nullptr, 1000.0, 1000.0,
                        dev<float>(), dev<float>(), 5, parents.data(), 16, 2, 3, 2000.0, 150.0, dev<void>(), wsb, dev<float>(), dev<int32_t>(),
                        dev<double>(), MPL_RPSM_ALL, nullptr) < 0);              // 0 < limb_stride < joints
    }
}

static mpl_synth_options synth_options() {
    mpl_synth_options o;
    std::memset(&o, 0, sizeof(o));
    o.penalize = MPL_SYNTH_PENALIZE_EXP_ERROR;
    o.clip = o.rotate = o.room = o.normalize_inputs = o.normalize_cameras = 1;
    o.noise_level = 2.0;
    o.missing_level = 0.05;
    o.penalize_a = 1.0, o.penalize_b = 0.1;
    o.room_min_x = o.room_min_y = -1000.0, o.room_max_x = o.room_max_y = 1000.0;
    o.img_w = o.img_h = 1000.0;
    for (int k = 0; k < 3; ++k) o.target_scale[k] = 1000.0;
    o.key_rot = 1, o.key_room_x = 2, o.key_room_y = 3, o.key_noise0 = 4, o.key_noise1 = 5, o.key_missing = 6;
    o.first_index = 1000003;
    return o;
}

static void walk_inputs_and_synthesis() {
    {
        auto call = [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
            std::vector<float*> lists(len(V), dev<float>());
            return mpl_prepare_inputs_ex(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<double>()), P(3, dev<double>()), B, V, J, 1000.f, 1000.f, 1, 1,
                                         P(4, lists.data()), P(5, lists.data()), P(6, lists.data()), nullptr);
        };
        walk("mpl_prepare_inputs_ex", 7, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 0}}, call);
        std::vector<float*> lists(4, dev<float>());
        lists[3] = nullptr;
        EXPECT(mpl_prepare_inputs_ex(dev<float>(), nullptr, dev<double>(), dev<double>(), 8, 4, 17, 1000.f, 1000.f, 1, 1, lists.data(), lists.data(),
                                     lists.data(), nullptr) < 0);
        lists[3] = dev<float>();
        EXPECT(mpl_prepare_inputs_ex(dev<float>(), nullptr, dev<double>(), dev<double>(), 8, 4, 17, 0.f, 1000.f, 1, 1, lists.data(), lists.data(),
                                     lists.data(), nullptr) < 0);
    }
    for (int ex = 0; ex < 2; ++ex) {
        auto call = [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
            std::vector<float*> lists(len(V), dev<float>());
            std::vector<mpl_synth_options> opt(1, synth_options());          // the struct on the heap at its own size
            if (ex)
                return mpl_synthesize_views_ex(P(0, dev<float>()), P(1, dev<double>()), P(2, dev<double>()), P(3, opt.data()), P(4, dev<float>()),
                                               P(5, dev<float>()), P(6, dev<float>()), P(7, dev<float>()), P(8, dev<float>()), B, V, J, P(9, lists.data()),
                                               P(10, lists.data()), P(11, lists.data()), P(12, dev<float>()), P(13, dev<float>()), P(14, dev<float>()),
                                               P(15, dev<float>()), nullptr);
            return mpl_synthesize_views(P(0, dev<float>()), P(1, dev<double>()), P(3, opt.data()), P(4, dev<float>()), P(5, dev<float>()),
                                        P(6, dev<float>()), P(7, dev<float>()), P(8, dev<float>()), B, V, J, P(9, lists.data()), P(10, lists.data()),
                                        P(11, lists.data()), P(12, dev<float>()), P(13, dev<float>()), P(14, dev<float>()), P(15, dev<float>()), nullptr);
        };
        walk(ex ? "mpl_synthesize_views_ex" : "mpl_synthesize_views", 16, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 0}}, call);
    }
    {
        std::vector<mpl_synth_options> opt(1, synth_options());
        opt[0].penalize = 4;
        EXPECT(mpl_synthesize_views(dev<float>(), dev<double>(), opt.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 8, 4, 17, nullptr, nullptr, nullptr,
                                    dev<float>(), nullptr, nullptr, nullptr, nullptr) < 0);
        opt[0] = synth_options();
        opt[0].target_scale[1] = 0.0;
        EXPECT(mpl_synthesize_views(dev<float>(), dev<double>(), opt.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 8, 4, 17, nullptr, nullptr, nullptr,
                                    dev<float>(), nullptr, nullptr, nullptr, nullptr) < 0);
        opt[0] = synth_options();
        EXPECT(mpl_synthesize_views(dev<float>(), dev<double>(), opt.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 8, 4, 17, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr) < 0);       // no output
        EXPECT(mpl_synthesize_views_ex(dev<float>(), dev<double>(), dev<double>(), opt.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 1 << 30, 32, 64,
                                       nullptr, nullptr, nullptr, dev<float>(), nullptr, nullptr, nullptr, nullptr) < 0);       // 2^41 items
    }
    for (int direction : {MPL_DISTORT_REMOVE, MPL_DISTORT_APPLY, 2}) {
        auto call = [&]() {
            return mpl_undistort_points(P(0, dev<float>()), P(1, dev<double>()), P(2, dev<double>()), S(0, 8), S(1, 4), S(2, 17), direction,
                                        P(3, dev<float>()), P(4, dev<unsigned char>()), nullptr);
        };
        walk("mpl_undistort_points", 5, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 0}}, call);
    }
}

static void walk_lines_of_sight() {
    for (int stride : {1, 3, 2}) {
        auto lists = [&](int V) { return std::vector<const float*>(len(V), dev<float>()); };
        walk("mpl_triangulate_rays", 5, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}}, [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
            auto r = lists(V), c = lists(V), w = lists(V);
            return mpl_triangulate_rays(P(0, r.data()), P(1, c.data()), P(2, w.data()), stride, B, V, J, P(3, dev<float>()), P(4, dev<float>()), nullptr);
        });
        walk("mpl_epipolar_errors", 6, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}}, [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
            auto r = lists(V), c = lists(V), w = lists(V);
            return mpl_epipolar_errors(P(0, r.data()), P(1, c.data()), P(2, w.data()), stride, B, V, J, P(3, dev<float>()), P(4, dev<float>()), 50.f,
                                       P(5, dev<float>() + 64), nullptr);
        });
        walk("mpl_triangulate_robust", 6, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 4}}, [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
            auto r = lists(V), c = lists(V), w = lists(V);
            return mpl_triangulate_robust(P(0, r.data()), P(1, c.data()), P(2, w.data()), stride, B, V, J, 30.0, 0.5, S(3, 2), P(3, dev<float>()),
                                          P(4, dev<float>()), P(5, dev<float>()), nullptr);
        });
    }
    std::vector<const float*> r(4, dev<float>()), hole(4, dev<float>());
    hole[3] = nullptr;
    EXPECT(mpl_triangulate_rays(hole.data(), r.data(), nullptr, 1, 8, 4, 17, dev<float>(), dev<float>(), nullptr) < 0);
    EXPECT(mpl_triangulate_rays(r.data(), hole.data(), nullptr, 1, 8, 4, 17, dev<float>(), dev<float>(), nullptr) < 0);
    EXPECT(mpl_triangulate_rays(r.data(), r.data(), hole.data(), 3, 8, 4, 17, dev<float>(), dev<float>(), nullptr) < 0);
    EXPECT(mpl_epipolar_errors(r.data(), r.data(), nullptr, 1, 8, 1, 17, dev<float>(), nullptr, 0.f, nullptr, nullptr) < 0);          // one view
    EXPECT(mpl_epipolar_errors(r.data(), r.data(), nullptr, 1, 8, 4, 17, dev<float>(), dev<float>(), 0.f, nullptr, nullptr) < 0);     // weight_in alone
    EXPECT(mpl_triangulate_robust(r.data(), r.data(), nullptr, 1, 8, 4, 17, 30.0, 0.5, 2, dev<float>(), dev<float>(), dev<float>(), nullptr) < 0);
    EXPECT(mpl_triangulate_robust(r.data(), r.data(), r.data(), 1, 8, 4, 17, 30.0, 65.0, 2, dev<float>(), dev<float>(), dev<float>(), nullptr) < 0);
    EXPECT(mpl_triangulate_robust(r.data(), r.data(), r.data(), 1, 1 << 30, 4, 64, 30.0, 0.5, 2, dev<float>(), dev<float>(), dev<float>(), nullptr) < 0);
}

static void walk_refinements() {
    walk("mpl_refine_points", 10, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 1000}}, [&]() {
        return mpl_refine_points(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<float>()), P(3, dev<double>()), P(4, dev<double>()), S(0, 8), S(1, 4),
                                 S(2, 17), 2.5, S(3, 10), 1e-9, P(5, dev<float>()), P(6, dev<float>()), P(7, dev<float>()), P(8, dev<int>()),
                                 P(9, dev<unsigned char>()), nullptr);
    });
    walk("mpl_refine_cameras", 12, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 1000}}, [&]() {
        return mpl_refine_cameras(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<float>()), P(3, dev<double>()), P(4, dev<double>()), S(0, 8), S(1, 4),
                                  S(2, 17), 2.5, S(3, 10), 1e-9, ~0u, P(5, dev<double>()), P(6, dev<double>()), P(7, dev<double>()), P(8, dev<double>()),
                                  P(9, dev<int>()), P(10, dev<int>()), P(11, dev<unsigned char>()), nullptr);
    });
    walk("mpl_refine_poses", 14, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 1000}}, [&]() {
        const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
        std::vector<int> parents(len(J, 64));
        for (size_t j = 0; j < parents.size(); ++j) parents[j] = (int)j - 1;
        return mpl_refine_poses(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<float>()), P(3, dev<double>()), P(4, dev<double>()), P(5, dev<float>()),
                                SL(4, J), P(6, parents.data()), B, V, J, 2.5, 100.0, S(3, 10), 1e-9, P(7, dev<float>()), P(8, dev<float>()),
                                P(9, dev<float>()), P(10, dev<double>()), P(11, dev<double>()), P(12, dev<int>()), P(13, dev<unsigned char>()), nullptr);
    });
    for (int kind = 0; kind < 5; ++kind) {
        std::vector<int> parents(17);
        for (int j = 0; j < 17; ++j) parents[j] = j - 1;
        if (kind == 0) parents[5] = -1;
        if (kind == 1) parents[0] = 3;
        if (kind == 2) parents[16] = 17;
        if (kind == 3) parents[16] = -2;
        if (kind == 4) parents[3] = 9, parents[9] = 3;
        EXPECT(mpl_refine_poses(dev<float>(), dev<float>(), nullptr, dev<double>(), nullptr, dev<float>(), 0, parents.data(), 8, 4, 17, 0.0, 100.0, 10, 1e-9,
                                dev<float>(), dev<float>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0);
    }
    for (double tol : {-1.0, (double)__builtin_nanf(""), (double)__builtin_inff()})
        EXPECT(mpl_refine_points(dev<float>(), dev<float>(), nullptr, dev<double>(), nullptr, 8, 4, 17, 0.0, 10, tol, dev<float>(), dev<float>(), nullptr,
                                 nullptr, nullptr, nullptr) < 0);
    EXPECT(mpl_refine_cameras(dev<float>(), dev<float>(), nullptr, dev<double>(), nullptr, 1 << 20, 32, 64, 0.0, 10, 1e-9, 0u, dev<double>(), dev<double>(),
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) < 0);                  // 2^31 observations
}

static void walk_hypothesise_and_score() {
    walk("mpl_locate_cameras", 15, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 65536}}, [&]() {
        const int B = S(0, 8), V = S(1, 4), J = S(2, 17);
        std::vector<unsigned long long> keys(len(V, MPL_MAX_VIEWS), 99ull);
        return mpl_locate_cameras(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<float>()), P(3, dev<double>()), P(4, dev<double>()), B, V, J, 5.0,
                                  S(3, 64), P(5, keys.data()), 1u, P(6, WS(dev<void>())), WSB(mpl_locate_cameras_workspace_bytes(B, V, J)), P(7, dev<double>()),
                                  P(8, dev<float>()), P(9, dev<int>()), P(10, dev<int>()), P(11, dev<double>()), P(12, dev<unsigned char>()),
                                  P(13, dev<double>()), P(14, dev<double>()), nullptr);
    });
    for (int n_pairs : {1, 3, MPL_MAX_VIEWS})
        walk("mpl_relative_pose", 18, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 65536}, {4, MPL_MAX_VIEWS}}, [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17), n = S(4, n_pairs);
            std::vector<int> pairs(2 * len(n, MPL_MAX_VIEWS));
            for (size_t i = 0; i < pairs.size(); i += 2) pairs[i] = (int)(i / 2) % 3, pairs[i + 1] = 3;
            std::vector<unsigned long long> keys(len(n, MPL_MAX_VIEWS), 99ull);
            return mpl_relative_pose(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<double>()), P(3, dev<double>()), B, V, J, P(4, pairs.data()), n, 5.0,
                                     S(3, 64), P(5, keys.data()), 1.0, P(6, WS(dev<void>())), WSB(mpl_relative_pose_workspace_bytes(B, n, J)), P(7, dev<double>()),
                                     P(8, dev<double>()), P(9, dev<double>()), P(10, dev<float>()), P(11, dev<int>()), P(12, dev<int>()), P(13, dev<double>()),
                                     P(14, dev<unsigned char>()), P(15, dev<double>()), P(16, dev<double>()), P(17, dev<int>()), nullptr);
        });
    for (int n_pairs : {1, 3, MPL_MAX_VIEWS})
        walk("mpl_refine_relative_pose", 17, {{0, 0}, {1, MPL_MAX_VIEWS}, {2, 64}, {3, 1000}, {4, MPL_MAX_VIEWS}}, [&]() {
            const int B = S(0, 8), V = S(1, 4), J = S(2, 17), n = S(4, n_pairs);
            std::vector<int> pairs(2 * len(n, MPL_MAX_VIEWS));
            for (size_t i = 0; i < pairs.size(); i += 2) pairs[i] = 3, pairs[i + 1] = (int)(i / 2) % 3;
            return mpl_refine_relative_pose(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<float>()), P(3, dev<double>()), P(4, dev<double>()), B, V, J,
                                            P(5, pairs.data()), n, P(6, dev<double>()), P(7, dev<double>()), 2.5, S(3, 10), 1e-9, 1.0, P(8, dev<double>()),
                                            P(9, dev<double>()), P(10, dev<double>()), P(11, dev<double>()), P(12, dev<double>()), P(13, dev<double>()),
                                            P(14, dev<int>()), P(15, dev<int>()), P(16, dev<unsigned char>()), nullptr);
        });
    // pairs that are not two distinct views of the call, each in a table of exactly 2 * n_pairs ints; workspaces that do not do
    const size_t wsb = mpl_relative_pose_workspace_bytes(8, 3, 17), lwb = mpl_locate_cameras_workspace_bytes(8, 4, 17);
    EXPECT(wsb > 0 && lwb > 0);
    std::vector<unsigned long long> keys3(3, 5ull), keys4(4, 5ull);
    std::vector<char> wsmem(wsb + lwb + 64);
    for (int kind = 0; kind < 7; ++kind) {
        std::vector<int> pairs{0, 1, 1, 2, 2, 3};
        if (kind == 0) pairs[5] = 4;            // names view V
        if (kind == 1) pairs[2] = 2;            // a == b
        if (kind == 2) pairs[0] = -1;
        if (kind == 3) pairs[4] = 2147483647;
        void* ws = kind == 5 ? (void*)(wsmem.data() + 1) : (void*)wsmem.data();
        const size_t bytes = kind == 4 ? wsb - 1 : kind == 6 ? 0 : wsb;
        EXPECT(mpl_relative_pose(dev<float>(), nullptr, dev<double>(), nullptr, 8, 4, 17, pairs.data(), 3, 5.0, 64, keys3.data(), 1.0, ws, bytes, dev<double>(),
                                 dev<double>(), dev<double>(), dev<float>(), dev<int>(), dev<int>(), dev<double>(), dev<unsigned char>(), dev<double>(),
                                 dev<double>(), dev<int>(), nullptr) < 0);
        if (kind < 4)
            EXPECT(mpl_refine_relative_pose(dev<float>(), nullptr, nullptr, dev<double>(), nullptr, 8, 4, 17, pairs.data(), 3, dev<double>(), dev<double>(), 0.0,
                                            10, 1e-9, 1.0, dev<double>(), dev<double>(), dev<double>(), dev<double>(), nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr) < 0);
        else
            EXPECT(mpl_locate_cameras(dev<float>(), dev<float>(), nullptr, dev<double>(), nullptr, 8, 4, 17, 5.0, 64, keys4.data(), 0u, ws,
                                      kind == 4 ? lwb - 1 : kind == 6 ? 0 : lwb, dev<double>(), dev<float>(), dev<int>(), dev<int>(), dev<double>(),
                                      dev<unsigned char>(), dev<double>(), dev<double>(), nullptr) < 0);
    }
    for (double bad : {0.0, -1.0, (double)__builtin_nanf(""), (double)__builtin_inff()}) {
        std::vector<int> pairs{0, 1};
        EXPECT(mpl_relative_pose(dev<float>(), nullptr, dev<double>(), nullptr, 8, 4, 17, pairs.data(), 1, bad, 64, keys3.data(), 1.0, wsmem.data(), wsb,
                                 dev<double>(), dev<double>(), dev<double>(), dev<float>(), dev<int>(), dev<int>(), dev<double>(), dev<unsigned char>(),
                                 dev<double>(), dev<double>(), dev<int>(), nullptr) < 0);
        EXPECT(mpl_locate_cameras(dev<float>(), dev<float>(), nullptr, dev<double>(), nullptr, 8, 4, 17, bad, 64, keys4.data(), 0u, wsmem.data(), lwb,
                                  dev<double>(), dev<float>(), dev<int>(), dev<int>(), dev<double>(), dev<unsigned char>(), dev<double>(), dev<double>(),
                                  nullptr) < 0);
    }
}

static std::vector<int> segments_of(long long frames, long long n_segments) {
    // n_segments lengths of at least 1 that sum to frames, none above MPL_SMOOTH_MAX_SEGMENT where that can be done
    std::vector<int> seg(len(n_segments, 1 << 16));
    long long left = frames;
    for (size_t i = 0; i < seg.size(); ++i) {
        const long long rest = (long long)seg.size() - 1 - (long long)i;
        long long take = i + 1 == seg.size() ? left : left / (rest + 1);
        if (take > MPL_SMOOTH_MAX_SEGMENT && i + 1 != seg.size()) take = MPL_SMOOTH_MAX_SEGMENT;
        if (take < 1) take = 1;
        seg[i] = (int)(take > 2147483647ll ? 2147483647ll : take);
        left -= take;
    }
    return seg;
}

static void walk_smooth_tracks() {
    std::vector<double> wsmem(4096);
    for (int order : {1, 2, 3}) {
        walk("mpl_smooth_tracks", 13, {{0, 0}, {2, MPL_SMOOTH_MAX_JOINTS}, {3, 1000}}, [&]() {
            const long long T = 300;
            const int n = S(0, 7), J = S(2, 17);
            std::vector<int> seg = segments_of(T, n);
            return mpl_smooth_tracks(P(0, dev<float>()), P(1, dev<float>()), P(2, seg.data()), P(3, dev<int>()), n, T, J, 10.0, order, 0.05, S(3, 20), 1e-6, 0u,
                                     P(4, WS((void*)wsmem.data())), WSB(mpl_smooth_tracks_workspace_bytes(T, J, n)), P(5, dev<float>()), P(6, dev<float>()),
                                     P(7, dev<float>()), P(8, dev<double>()), P(9, dev<double>()), P(10, dev<int>()), P(11, dev<unsigned char>()),
                                     P(12, dev<double>()), nullptr);
        });
    }
    // frames: 0, negative, the limit (256 segments of the longest kind), the limit + 1, beyond int
    for (long long T : {0ll, -1ll, (long long)MPL_SMOOTH_MAX_FRAMES, (long long)MPL_SMOOTH_MAX_FRAMES + 1, 1ll << 31, (1ll << 32) + 300, 1ll << 62}) {
        const long long n = T > 0 ? (T + MPL_SMOOTH_MAX_SEGMENT - 1) / MPL_SMOOTH_MAX_SEGMENT : 1;
        std::vector<int> seg = segments_of(T, n);
        EXPECT(mpl_smooth_tracks(dev<float>(), nullptr, seg.data(), dev<int>(), (int)(n > 2147483647ll ? 2147483647ll : n), T, 17, 10.0, 2, 0.0, 20, 1e-6, 0u,
                                 wsmem.data(), mpl_smooth_tracks_workspace_bytes(T, 17, (int)(n > 2147483647ll ? 2147483647ll : n)), dev<float>(), dev<float>(),
                                 dev<float>(), dev<double>(), dev<double>(), dev<int>(), dev<unsigned char>(), nullptr, nullptr) < 0);
    }
    const size_t wsb = mpl_smooth_tracks_workspace_bytes(300, 17, 3);
    EXPECT(wsb > 0);
    for (int kind = 0; kind < 9; ++kind) {
        std::vector<int> seg{100, 100, 100};
        long long T = 300;
        if (kind == 0) seg[1] = 0, seg[2] = 200;                                  // a segment of 0
        if (kind == 1) seg[2] = 99;                                               // does not sum to frames
        if (kind == 2) seg[2] = 101;
        if (kind == 3) seg[0] = -100, seg[1] = 300;                               // sums, with a negative entry
        if (kind == 4) seg = {MPL_SMOOTH_MAX_SEGMENT + 1, 100, 100}, T = MPL_SMOOTH_MAX_SEGMENT + 201;
        if (kind == 5) seg = {2147483647, 2147483647, 2}, T = 300;                // wraps to 0 in int, to 2^32 in unsigned
        void* ws = kind == 7 ? (void*)((char*)wsmem.data() + 4) : (void*)wsmem.data();
        const size_t bytes = kind == 6 ? wsb - 1 : kind == 8 ? 0 : mpl_smooth_tracks_workspace_bytes(T, 17, 3);
        EXPECT(mpl_smooth_tracks(dev<float>(), nullptr, seg.data(), dev<int>(), 3, T, 17, 10.0, 2, 0.0, 20, 1e-6, 0u, ws, bytes, dev<float>(), dev<float>(),
                                 dev<float>(), dev<double>(), dev<double>(), dev<int>(), dev<unsigned char>(), nullptr, nullptr) < 0);
    }
    std::vector<int> seg{100, 100, 100};
    for (double smooth : {0.0, -1.0, (double)__builtin_nanf(""), (double)__builtin_inff()})
        EXPECT(mpl_smooth_tracks(dev<float>(), nullptr, seg.data(), dev<int>(), 3, 300, 17, smooth, 2, 0.0, 20, 1e-6, 0u, wsmem.data(), wsb, dev<float>(),
                                 dev<float>(), dev<float>(), dev<double>(), dev<double>(), dev<int>(), dev<unsigned char>(), nullptr, nullptr) < 0);
    for (unsigned flags : {MPL_SMOOTH_F_SINGLE_LANE, 2u, ~0u})
        EXPECT(mpl_smooth_tracks(dev<float>(), nullptr, seg.data(), dev<int>(), 3, 300, 17, 10.0, 2, 0.0, 20, 1e-6, flags, wsmem.data(), wsb, dev<float>(),
                                 dev<float>(), dev<float>(), dev<double>(), dev<double>(), dev<int>(), dev<unsigned char>(), nullptr, nullptr) < 0);
    EXPECT(mpl_smooth_tracks(dev<float>(), nullptr, seg.data(), dev<int>(), 301, 300, 17, 10.0, 2, 0.0, 20, 1e-6, 0u, wsmem.data(), wsb, dev<float>(), dev<float>(),
                             dev<float>(), dev<double>(), dev<double>(), dev<int>(), dev<unsigned char>(), nullptr, nullptr) < 0);       // more segments than frames
}

static void walk_procrustes_and_evaluator() {
    for (int reflection : {0, 1, 2, 3}) {
        walk("mpl_procrustes_align", 11, {{0, 0}, {1, 64}, {2, 64}}, [&]() {
            const int B = S(0, 8), J = S(1, 17), n_sel = S(2, 14);
            std::vector<int> sel(len(n_sel, 64));
            for (size_t k = 0; k < sel.size(); ++k) sel[k] = (int)k % (J > 0 ? J : 1);
            std::vector<float> s3(3, 1000.f), o3(3, 0.f);
            return mpl_procrustes_align(P(0, dev<float>()), P(1, dev<float>()), P(2, dev<float>()), P(3, sel.data()), n_sel, P(4, s3.data()), P(5, o3.data()), 1,
                                        reflection, B, J, P(6, dev<float>()), P(7, dev<float>()), P(8, dev<float>()), P(9, dev<float>()), P(10, dev<float>()),
                                        nullptr);
        });
    }
    for (int bad : {17, -1, 2147483647}) {
        std::vector<int> sel{0, 1, 2, bad};
        EXPECT(mpl_procrustes_align(dev<float>(), dev<float>(), nullptr, sel.data(), 4, nullptr, nullptr, 1, 0, 8, 17, dev<float>(), dev<float>(), nullptr, nullptr,
                                    nullptr, nullptr) < 0);
    }
    EXPECT(mpl_procrustes_align(dev<float>(), dev<float>(), nullptr, nullptr, 0, nullptr, nullptr, 1, 0, 8, 17, nullptr, nullptr, dev<float>(), nullptr, nullptr,
                                nullptr) < 0);            // neither aligned nor d
    EXPECT(mpl_procrustes_align(dev<float>(), dev<float>(), nullptr, nullptr, 0, nullptr, nullptr, 1, 0, 1 << 26, 64, dev<float>(), nullptr, nullptr, nullptr,
                                nullptr, nullptr) < 0);   // 2^32 joints in all

    walk("mpl_eval_reset", 1, {{0, 64}, {1, MPL_EVAL_MAX_GROUPS}},
         [&]() { return mpl_eval_reset(P(0, dev<void>()), S(0, 17), S(1, 3), nullptr); });
    walk("mpl_eval_report", 2, {{0, 64}, {1, MPL_EVAL_MAX_GROUPS}},
         [&]() { return mpl_eval_report(P(0, (const void*)dev<void>()), S(0, 17), S(1, 3), ~0ull, P(1, dev<double>()), nullptr); });
    for (int crit = -1; crit <= 5; ++crit)
        for (int axis = 0; axis < 2; ++axis)
            walk("mpl_eval_accumulate", 11, {{0, 0}, {1, 64}, {2, 64}, {3, MPL_EVAL_MAX_GROUPS}, {4, 0}}, [&]() {
                const int B = S(0, 17), J = S(1, 17);
                std::vector<mpl_eval_options> opt(1);
                std::memset(opt.data(), 0, sizeof(mpl_eval_options));
                opt[0].criterion = crit;
                opt[0].has_weight_axis = axis;
                for (int k = 0; k < 3; ++k) opt[0].weight_axis[k] = 1.f, opt[0].scale[k] = 1000.f;
                opt[0].metre_factor = 100.f;
                opt[0].n_views = 4;
                opt[0].n_sel = S(2, 14);
                opt[0].n_groups = S(3, 3);
                for (int k = 0; k < 64; ++k) opt[0].sel[k] = (uint8_t)(k % (J > 0 && J < 255 ? J : 1));
                return mpl_eval_accumulate(P(0, dev<void>()), P(1, opt.data()), P(2, dev<float>()), P(3, dev<float>()), P(4, dev<float>()), P(5, dev<float>()),
                                           P(6, dev<float>()), P(7, dev<float>()), P(8, dev<int32_t>()), B, J, P(9, dev<float>()), P(10, dev<float>()),
                                           SL(4, 100), nullptr);
            });
    {
        std::vector<mpl_eval_options> opt(1);
        std::memset(opt.data(), 0, sizeof(mpl_eval_options));
        opt[0].n_sel = 14, opt[0].n_groups = 1, opt[0].n_views = 4, opt[0].metre_factor = 1.f;
        for (int k = 0; k < 64; ++k) opt[0].sel[k] = 255;                        // a selection beyond the joints
        EXPECT(mpl_eval_accumulate(dev<void>(), opt.data(), dev<float>(), nullptr, nullptr, dev<float>(), nullptr, nullptr, nullptr, 8, 17, nullptr, nullptr, 0,
                                   nullptr) < 0);
        for (int k = 0; k < 64; ++k) opt[0].sel[k] = (uint8_t)(k % 17);
        EXPECT(mpl_eval_accumulate(dev<void>(), opt.data(), dev<float>(), nullptr, nullptr, dev<float>(), nullptr, nullptr, nullptr, 8, 17, dev<float>(), nullptr,
                                   100, nullptr) < 0);      // keep_pred without keep_tgt
        EXPECT(mpl_eval_accumulate(dev<void>(), opt.data(), dev<float>(), nullptr, nullptr, dev<float>(), nullptr, nullptr, nullptr, 8, 17, dev<float>(),
                                   dev<float>(), -1, nullptr) < 0);
    }
}

static void walk_bf16_any() {
    std::vector<uint16_t> dst(1 << 12, 0);
    for (int ln = 0; ln < 2; ++ln) {
        walk("mpl_pack_bf16_any", 5, {{0, 0}, {1, 0}}, [&]() {
            return mpl_pack_bf16_any(P(0, dev<float>()), P(1, dev<float>()), ln ? P(2, dev<float>()) : nullptr, ln ? P(3, dev<float>()) : nullptr, S(0, 480),
                                     S(1, 480), P(4, dst.data()), nullptr);
        });
        walk("mpl_ln_linear_bf16_any", 6, {{0, 0}, {1, 0}, {2, 0}}, [&]() {
            const int M = S(0, 12), K = S(1, 480), N = S(2, 960);
            return mpl_ln_linear_bf16_any(P(0, dev<float>()), M, K, ln, 1e-6f, P(1, dst.data()), N, ln ? MPL_EPI_BIAS_GELU : MPL_EPI_BIAS_RESIDUAL,
                                          P(2, dev<float>()), P(3, dev<void>()), P(4, dev<float>()), P(5, WS(dev<void>())),
                                          WSB(mpl_ln_linear_bf16_any_workspace_bytes(M, K)), nullptr);
        });
    }
    const size_t wsb = mpl_ln_linear_bf16_any_workspace_bytes(12, 480);
    for (int kind = 0; kind < 4; ++kind)
        EXPECT(mpl_ln_linear_bf16_any(dev<float>(), 12, 480, 1, 1e-6f, dst.data(), 960, kind == 3 ? 9 : MPL_EPI_BIAS, nullptr, dev<void>(), dev<float>(),
                                      kind == 1 ? (void*)((char*)g_fake.data() + 1) : dev<void>(), kind == 0 && wsb ? wsb - 1 : kind == 2 ? 0 : wsb, nullptr) < 0);
    EXPECT(mpl_pack_bf16_any(dev<float>(), dev<float>(), dev<float>(), nullptr, 480, 480, dst.data(), nullptr) < 0);      // ln_w without ln_b
    EXPECT(mpl_pack_bf16_any(dev<float>(), dev<float>(), nullptr, nullptr, 480, 480, (uint16_t*)((char*)dst.data() + 2), nullptr) < 0);   // not 16-byte aligned
}

int main() {
    // the calls below hand the library host pointers, and its device code is empty bundles here: it must never meet a device
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        std::fprintf(stderr, "host_driver: %d GPU(s) visible, this job needs none (run.sh sets HIP_VISIBLE_DEVICES=-1)\n", devices);
        return 2;
    }
    EXPECT(mpl_hip_abi_version() == MPL_HIP_ABI_VERSION);
    for (int c = -9; c <= 1; ++c) {
        const char* s = mpl_hip_error_string(c);
        EXPECT(s != nullptr && std::strlen(s) > 0);
    }

    // ---- configuration queries: every flag combination, degenerate and huge batches
    for (unsigned f = 0; f < (1u << 13); f += 37) {
        mpl_config cfg{17, 32, 12, 8, 4, (f & 1) ? 3 : 2, f, 0};
        const int w = mpl_fpt_width(&cfg);
        EXPECT(w == 32 || w == 544 || w == 1088 || w < 0);
        for (int B : {0, 1, 3, 1024, 8192, 1 << 20}) (void)mpl_forward_workspace_bytes(&cfg, B);
    }
    {
        mpl_config bad{0, 0, 0, 0, 0, 0, 0, 0};
        (void)mpl_fpt_width(&bad);
        (void)mpl_forward_workspace_bytes(&bad, 16);
        (void)mpl_fpt_width(nullptr);
        (void)mpl_forward_workspace_bytes(nullptr, 16);
        mpl_config neg{17, 32, -1, 8, 4000, 2, 0, 0};
        (void)mpl_forward_workspace_bytes(&neg, -5);
    }
    for (int n_seq : {0, 1, 256, 1024, 1 << 22})
        for (int n_tok : {0, 1, 2, 4, 31, 32, 33, 527})
            for (int dim : {0, 32, 136, 544, 1088, 4352, 7}) (void)mpl_block_stack_workspace_bytes(n_seq, n_tok, dim);
    for (int N : {0, 51, 96, 136, 544, 1088, 1632, 2176, 3264})
        for (int K : {0, 32, 64, 100, 544, 1088, 2176}) {
            (void)mpl_pack_h2_bytes(N, K);
            (void)mpl_pack_bf16_bytes(N, K);
            (void)mpl_ln_linear_h2_workspace_bytes(N, K);
        }
    EXPECT(mpl_pack_h2_bytes(1632, 544) == (size_t)12 * 17 * 18 * 1024 + (5 * 1632 + 8) * 4);
    EXPECT(mpl_pack_bf16_bytes(544, 100) == 0);
    EXPECT(mpl_spt_pack_bytes() >= 34 * 1024);
    EXPECT(mpl_pose_metrics_size(17) > 0);
    (void)mpl_pose_metrics_size(0);
    (void)mpl_pose_metrics_size(-3);
    (void)mpl_pack_h2_out_scale(nullptr, 1632, 544);

    // ---- the launch rule query: invalid arguments are refused before any device query; valid ones need a device
    EXPECT(mpl_block_stack_form(0, 2, 544, 8, 13, 2, 0) < 0);
    EXPECT(mpl_block_stack_form(256, 0, 544, 8, 13, 2, 0) < 0);
    EXPECT(mpl_block_stack_form(256, 2, 0, 8, 13, 2, 0) < 0);
    EXPECT(mpl_block_stack_form(256, 2, 544, 0, 13, 2, 0) < 0);
    EXPECT(mpl_block_stack_form(256, 2, 544, 8, 0, 2, 0) < 0);
    EXPECT(mpl_block_stack_form(256, 2, 544, 8, 13, 7, 0) < 0);
    (void)mpl_block_stack_form(256, 2, 544, 8, 13, 2, 0);
    (void)mpl_block_stack_form(1, 2, 544, 8, 13, 2, MPL_F_NO_SMALL_STACK);
    (void)mpl_block_stack_form(1024, 4, 1088, 8, MPL_MAX_APPS + 5, 1, 0);
    EXPECT(mpl_block_stack_form_ex(1, 2, 544, 8, 13, 14, 1, 2, 0) < 0);       // more blocks than applications
    EXPECT(mpl_block_stack_form_ex(1, 2, 544, 8, 13, 0, 1, 2, 0) < 0);
    (void)mpl_block_stack_form_ex(1, 2, 544, 8, 13, 12, 0, 2, 0);
    EXPECT(mpl_block_stack_last_form() < 0);                                  // nothing was launched by this thread

    // ---- the SPT launch rule query: with the compute units given it needs no device
    {
        int spw = -1;
        mpl_config c17{17, 32, 2, 8, 3, 2, MPL_F_POS3D_LEARN, 0};
        EXPECT(mpl_spt_form(nullptr, 8, 1, 256, &spw) < 0 && spw == -1);
        EXPECT(mpl_spt_form(&c17, 0, 1, 256, &spw) < 0);
        EXPECT(mpl_spt_form(&c17, 900, 0, 256, &spw) == MPL_SPT_FRAGS && spw == 11);
        EXPECT(mpl_spt_form(&c17, 900, 1, 256, &spw) == MPL_SPT_PACKED && spw == 16);
        EXPECT(mpl_spt_form(&c17, 85, 0, 256, nullptr) == MPL_SPT_STAGED);
        c17.flags |= MPL_F_GENERIC_SPT;
        EXPECT(mpl_spt_form(&c17, 1 << 30, 1, 256, &spw) == MPL_SPT_ANY && spw >= 1);
        mpl_config c65{65, 32, 2, 8, 3, 2, MPL_F_POS3D_LEARN, 0};
        EXPECT(mpl_spt_form(&c65, 8, 0, 256, &spw) < 0);
        EXPECT(mpl_spt_form(&c17, 8, 0, 0, &spw) < 0);                           // asks the device: none here
    }

    // ---- switches and per-device state
    EXPECT(mpl_x3_spin_limit(0) < 0);
    EXPECT(mpl_x3_spin_limit(31) < 0);
    EXPECT(mpl_x3_spin_limit(-1) < 0);
    EXPECT(mpl_x3_spin_limit(23) == MPL_OK);
    for (int m = 0; m < 300; m += 7) (void)mpl_x3_stack_mode(m);
    (void)mpl_x3_stack_mode(0);
    (void)mpl_x3_debug_buffer(nullptr);
    for (int d : {-1, 0, 1, 63, 64, 1000}) {
        (void)mpl_device_error(d);
        (void)mpl_device_error_clear(d);
    }
    {
        float ms[16] = {0};
        int cnt[16] = {0};
        (void)mpl_profile_start();
        (void)mpl_profile_stop(ms, cnt, 16);
        (void)mpl_profile_stop(ms, cnt, 16);      // stop without start
        (void)mpl_profile_stop(nullptr, nullptr, 0);
    }

    // ---- whole-forward entry points: NULL / too small / inconsistent arguments, then well-formed calls without a device.
    // Device pointers are opaque to the host side (never dereferenced there): small host arrays stand in for them.
    std::vector<float> fake(4096, 0.f);
    std::vector<mpl_block_weights> blocks(12);
    std::memset(blocks.data(), 0, blocks.size() * sizeof(mpl_block_weights));
    for (auto& b : blocks) {
        b.ln1_w = b.ln1_b = b.qkv_w = b.qkv_b = b.proj_w = b.proj_b = fake.data();
        b.ln2_w = b.ln2_b = b.fc1_w = b.fc1_b = b.fc2_w = b.fc2_b = fake.data();
    }
    mpl_spt_set set{fake.data(), fake.data(), nullptr, nullptr, fake.data(), blocks.data()};
    mpl_weights w;
    std::memset(&w, 0, sizeof(w));
    w.spt_sets = &set;
    w.spatial_norm_w = w.spatial_norm_b = w.pos_3d_embed = w.pos_3d_view_coding = fake.data();
    w.pos_3d_linear_w = w.pos_3d_linear_b = w.view_norm_w = w.view_norm_b = w.wmean_w = w.wmean_b = fake.data();
    w.head_ln_w = w.head_ln_b = w.head_w = w.head_b = fake.data();
    w.fpt_blocks = blocks.data();
    mpl_inputs in;
    std::memset(&in, 0, sizeof(in));
    in.batch = 8;
    for (int v = 0; v < 4; ++v) in.poses[v] = in.rays[v] = in.centers[v] = fake.data();
    mpl_config cfg{17, 32, 12, 8, 4, 2, MPL_F_POS3D_LEARN, 0};
    const size_t wsb = mpl_forward_workspace_bytes(&cfg, 8);
    std::vector<char> ws(wsb + 256);
    EXPECT(mpl_forward(nullptr, &w, &in, fake.data(), ws.data(), wsb, nullptr) < 0);
    EXPECT(mpl_forward(&cfg, nullptr, &in, fake.data(), ws.data(), wsb, nullptr) < 0);
    EXPECT(mpl_forward(&cfg, &w, nullptr, fake.data(), ws.data(), wsb, nullptr) < 0);
    EXPECT(mpl_forward(&cfg, &w, &in, nullptr, ws.data(), wsb, nullptr) < 0);
    EXPECT(mpl_forward(&cfg, &w, &in, fake.data(), nullptr, wsb, nullptr) < 0);
    EXPECT(mpl_forward(&cfg, &w, &in, fake.data(), ws.data(), wsb / 2, nullptr) < 0);
    {
        mpl_config c2 = cfg;
        c2.num_views = MPL_MAX_VIEWS + 1;
        EXPECT(mpl_forward(&c2, &w, &in, fake.data(), ws.data(), wsb, nullptr) < 0);
        c2 = cfg;
        c2.depth = MPL_MAX_APPS + 3;
        EXPECT(mpl_forward(&c2, &w, &in, fake.data(), ws.data(), wsb, nullptr) < 0);
        c2 = cfg;
        c2.num_joints = 18;
        EXPECT(mpl_forward(&c2, &w, &in, fake.data(), ws.data(), wsb, nullptr) < 0);
        c2 = cfg;
        c2.flags |= MPL_F_KPTOK | MPL_F_RAYS_TOKEN;
        EXPECT(mpl_forward(&c2, &w, &in, fake.data(), ws.data(), wsb, nullptr) < 0);
        mpl_inputs i2 = in;
        i2.batch = -4;
        EXPECT(mpl_forward(&cfg, &w, &i2, fake.data(), ws.data(), wsb, nullptr) < 0);
        i2 = in;
        i2.poses[2] = nullptr;
        EXPECT(mpl_forward(&cfg, &w, &i2, fake.data(), ws.data(), wsb, nullptr) < 0);
    }
    EXPECT(mpl_forward(&cfg, &w, &in, fake.data(), ws.data(), wsb, nullptr) < 0);      // well formed: no device here
    EXPECT(mpl_spt_tokens(&cfg, &w, &in, fake.data(), nullptr) < 0);
    EXPECT(mpl_fuse_head(&cfg, &w, fake.data(), 8, fake.data(), nullptr) < 0);
    EXPECT(mpl_view_fuse(&cfg, &w, fake.data(), 8, fake.data(), nullptr) < 0);
    EXPECT(mpl_view_norm(&cfg, &w, fake.data(), 8, fake.data(), nullptr) < 0);

    // ---- the block stack: schedules of every length, indices beyond the blocks, workspaces of every size
    {
        std::vector<uint8_t> sched(MPL_MAX_APPS + 8);
        for (size_t i = 0; i < sched.size(); ++i) sched[i] = (uint8_t)(i % 12);
        const size_t sb = mpl_block_stack_workspace_bytes(8, 4, 544);
        std::vector<char> sw(sb + 256);
        for (int n_apps : {-1, 0, 1, 13, MPL_MAX_APPS, MPL_MAX_APPS + 1, MPL_MAX_APPS + 8})
            for (size_t bytes : {(size_t)0, sb / 3, sb, sb + 100}) {
                EXPECT(mpl_block_stack(fake.data(), 8, 4, 544, 8, blocks.data(), sched.data(), n_apps, sw.data(), bytes, nullptr) < 0 || n_apps == 0);
                (void)mpl_block_stack_ex(fake.data(), 8, 4, 544, 8, blocks.data(), sched.data(), n_apps, sw.data(), bytes,
                                         MPL_F_NO_SMALL_STACK, nullptr);
            }
        EXPECT(mpl_block_stack(nullptr, 8, 4, 544, 8, blocks.data(), sched.data(), 13, sw.data(), sb, nullptr) < 0);
        EXPECT(mpl_block_stack(fake.data(), 8, 4, 544, 8, nullptr, sched.data(), 13, sw.data(), sb, nullptr) < 0);
        EXPECT(mpl_block_stack(fake.data(), 8, 4, 544, 8, blocks.data(), nullptr, 13, sw.data(), sb, nullptr) < 0);
        EXPECT(mpl_block_stack(fake.data(), 8, 4, 544, 7, blocks.data(), sched.data(), 13, sw.data(), sb, nullptr) < 0);
        EXPECT(mpl_block_stack(fake.data(), 8, 4, 545, 8, blocks.data(), sched.data(), 13, sw.data(), sb, nullptr) < 0);
        EXPECT(mpl_block_stack(fake.data(), 1 << 30, 4, 544, 8, blocks.data(), sched.data(), 13, sw.data(), sb, nullptr) < 0);
        // packed-operand blocks (fp16x2 / bf16 / d32 fields set): the engine selection paths of block_stack_impl
        std::vector<mpl_block_weights> pk = blocks;
        std::vector<uint16_t> op(1 << 16, 0);
        for (auto& b : pk) b.qkv_h2 = b.proj_h2 = b.fc1_h2 = b.fc2_h2 = op.data();
        (void)mpl_block_stack(fake.data(), 64, 4, 544, 8, pk.data(), sched.data(), 13, sw.data(), sb, nullptr);
        for (auto& b : pk) {
            b.qkv_h2 = b.proj_h2 = b.fc1_h2 = b.fc2_h2 = nullptr;
            b.qkv_w16 = b.proj_w16 = b.fc1_w16 = b.fc2_w16 = op.data();
        }
        (void)mpl_block_stack(fake.data(), 64, 4, 544, 8, pk.data(), sched.data(), 13, sw.data(), sb, nullptr);
        pk[3].fc1_w16 = nullptr;          // one block without its operand: the stack must not mix engines
        (void)mpl_block_stack(fake.data(), 64, 4, 544, 8, pk.data(), sched.data(), 13, sw.data(), sb, nullptr);
        std::vector<mpl_block_weights> d32 = blocks;
        for (auto& b : d32) b.qkv_w3 = op.data();
        (void)mpl_block_stack(fake.data(), 4, 68, 32, 8, d32.data(), sched.data(), 3, sw.data(), sb, nullptr);
    }

    // ---- the unit entry points
    EXPECT(mpl_ln_linear(fake.data(), 64, 544, fake.data(), fake.data(), 1e-6f, fake.data(), fake.data(), 544, MPL_EPI_BIAS, nullptr,
                         fake.data(), fake.data(), nullptr) < 0);
    EXPECT(mpl_ln_linear(nullptr, 64, 544, nullptr, nullptr, 1e-6f, fake.data(), fake.data(), 544, 9, nullptr, fake.data(), nullptr, nullptr) < 0);
    EXPECT(mpl_token_attention(fake.data(), 8, 4, 544, 8, fake.data(), nullptr) < 0);
    EXPECT(mpl_token_attention(fake.data(), 8, 4, 544, 7, fake.data(), nullptr) < 0);
    EXPECT(mpl_layernorm(fake.data(), 8, 544, fake.data(), fake.data(), 1e-5f, fake.data(), nullptr) < 0);
    EXPECT(mpl_linear(fake.data(), 51, fake.data(), 544, 8, fake.data(), fake.data(), 1024, nullptr, nullptr, nullptr, nullptr, 1e-5f, 1,
                      fake.data(), nullptr) < 0);
    EXPECT(mpl_linear(nullptr, 0, nullptr, 0, 8, fake.data(), fake.data(), 1024, nullptr, nullptr, nullptr, nullptr, 1e-5f, 0, fake.data(),
                      nullptr) < 0);
    {
        std::vector<uint16_t> dst(64 * 1024, 0);
        EXPECT(mpl_spt_pack(&blocks[0], dst.data(), nullptr) < 0);
        EXPECT(mpl_spt_pack(nullptr, dst.data(), nullptr) < 0);
        EXPECT(mpl_d32_pack(&blocks[0], nullptr, nullptr) < 0);
        EXPECT(mpl_pack_bf16(fake.data(), fake.data(), nullptr, nullptr, 544, 100, dst.data(), nullptr) < 0);
        EXPECT(mpl_pack_bf16(fake.data(), fake.data(), nullptr, nullptr, 544, 544, dst.data(), nullptr) < 0);
        EXPECT(mpl_pack_h2(fake.data(), fake.data(), fake.data(), fake.data(), 544, 2176, dst.data(), nullptr) < 0);
        EXPECT(mpl_pack_h2(fake.data(), fake.data(), nullptr, nullptr, 544, 544, dst.data(), nullptr) < 0);
        EXPECT(mpl_pack_h2_scaled(fake.data(), fake.data(), nullptr, 544, 544, dst.data(), nullptr) < 0);
        EXPECT(mpl_ln_linear_h2(fake.data(), 64, 544, 1, 1e-6f, dst.data(), 544, MPL_EPI_BIAS, nullptr, fake.data(), fake.data(), ws.data(),
                                16, nullptr) < 0);
    }
    {
        float* views[4] = {fake.data(), fake.data(), fake.data(), fake.data()};
        std::vector<double> cams(4 * 16, 0.0);
        EXPECT(mpl_prepare_inputs(fake.data(), nullptr, cams.data(), 8, 4, 17, 1000.f, 1000.f, 1, 0, views, views, views, nullptr) < 0);
        EXPECT(mpl_prepare_inputs(fake.data(), nullptr, cams.data(), 8, MPL_MAX_VIEWS + 1, 17, 1000.f, 1000.f, 1, 0, views, views, views, nullptr) < 0);
        EXPECT(mpl_prepare_inputs(nullptr, nullptr, cams.data(), 8, 4, 17, 1000.f, 1000.f, 1, 0, views, views, views, nullptr) < 0);
        const float sc[3] = {1.f, 2.f, 3.f};
        EXPECT(mpl_pose_metrics(fake.data(), fake.data(), nullptr, 8, 17, sc, sc, fake.data(), nullptr) < 0);
        EXPECT(mpl_pose_metrics_ex(fake.data(), fake.data(), fake.data(), 8, 17, nullptr, nullptr, 0x1ffffu, fake.data(), nullptr) < 0);
        EXPECT(mpl_pose_metrics(nullptr, fake.data(), nullptr, 8, 17, sc, sc, fake.data(), nullptr) < 0);
        EXPECT(mpl_pose_metrics(fake.data(), fake.data(), nullptr, 8, 40, sc, sc, fake.data(), nullptr) < 0);
    }
    walk_queries();
    walk_heatmaps();
    walk_inputs_and_synthesis();
    walk_lines_of_sight();
    walk_refinements();
    walk_hypothesise_and_score();
    walk_smooth_tracks();
    walk_procrustes_and_evaluator();
    walk_bf16_any();
    std::printf("host_driver: %d expectation(s) failed\n", failures);
    return failures ? 1 : 0;
}
