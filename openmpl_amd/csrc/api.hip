// C ABI of libmpl_hip.so (include/mpl_hip.h): argument validation + launch orchestration.
// One mpl_forward call enqueues the whole forward on the caller's stream; nothing synchronises.
#include "common.hpp"

#include <stdlib.h>

#include <mutex>
#include <vector>

using namespace mpl;

// ------------------------------------------------------------------ profiling aid
// The only process-global mutable state of the library besides the set-once function-attribute flags: a list of event
// pairs, guarded by a mutex (launches may come from one thread per GPU under DataParallel).  Off unless
// mpl_profile_start() was called; the fast path is one relaxed atomic load.
namespace {
struct ProfRec {
    hipEvent_t e0, e1;
    int kind;
};
std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof;
}  // namespace

mpl::ProfScope::ProfScope(int kind, hipStream_t s) : slot(-1), stream(s) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return;
    ProfRec r;
    r.kind = kind;
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return;
    hipEventRecord(r.e0, s);
    std::lock_guard<std::mutex> g(g_prof_mu);
    g_prof.push_back(r);
    slot = (int)g_prof.size() - 1;
}
mpl::ProfScope::~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> g(g_prof_mu);
    if (slot < (int)g_prof.size()) hipEventRecord(g_prof[slot].e1, stream);
}

// ------------------------------------------------------------------ device-side failure word (common.hpp)
namespace {
std::mutex g_err_mu;
unsigned* g_err_host[64];      // pinned host words, one per device, allocated on first use, never freed
unsigned* g_err_dev[64];       // the same words as the device addresses them
}  // namespace

unsigned* mpl::device_error_word(int dev) {
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> g(g_err_mu);
    if (!g_err_host[dev]) {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) return nullptr;
        *reinterpret_cast<volatile unsigned*>(h) = 0u;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) d = h;
        g_err_host[dev] = reinterpret_cast<unsigned*>(h);
        g_err_dev[dev] = reinterpret_cast<unsigned*>(d);
    }
    return g_err_dev[dev];
}
int mpl::device_error_pending(int dev) {
    if (dev < 0 || dev >= 64) return 0;
    std::lock_guard<std::mutex> g(g_err_mu);
    return g_err_host[dev] ? (int)*reinterpret_cast<volatile unsigned*>(g_err_host[dev]) : 0;
}
void mpl::device_error_clear(int dev) {
    if (dev < 0 || dev >= 64) return;
    std::lock_guard<std::mutex> g(g_err_mu);
    if (g_err_host[dev]) *reinterpret_cast<volatile unsigned*>(g_err_host[dev]) = 0u;
}

namespace {
std::atomic<int> g_fault_phase{0};
}  // namespace
void mpl::set_fault_injection(int phase) { g_fault_phase.store(phase); }
int mpl::take_fault_injection() { return g_fault_phase.exchange(0); }
int mpl::refuse_stream_capture(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return MPL_OK;                       // the legacy default stream cannot be queried while another stream captures
    }
    return st == hipStreamCaptureStatusNone ? MPL_OK : MPL_E_UNSUPPORTED;
}

namespace {
std::mutex g_chain_mu[64];
hipEvent_t g_chain_ev[64];
std::mutex g_chain_create_mu;
}  // namespace
std::mutex& mpl::stack_chain_mutex(int dev) { return g_chain_mu[(dev >= 0 && dev < 64) ? dev : 0]; }
hipEvent_t mpl::stack_chain_event(int dev) {
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> g(g_chain_create_mu);
    if (!g_chain_ev[dev] && hipEventCreateWithFlags(&g_chain_ev[dev], hipEventDisableTiming) != hipSuccess) g_chain_ev[dev] = nullptr;
    return g_chain_ev[dev];
}

namespace {
std::atomic<int> g_stack_mode{(getenv("MPL_X3_LAUNCHES") != nullptr ? 1 : 0) | (getenv("MPL_NO_SMALL_STACK") != nullptr ? 8 : 0) |
                              (getenv("MPL_WRITE_THROUGH") != nullptr ? 128 : 0)};     // mpl_x3_stack_mode: the bits at stack_mode()
}  // namespace
int mpl::stack_mode() { return g_stack_mode.load(); }

// compute units of the current device (asked once per device)
int mpl::device_cu_count(int* cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return MPL_E_LAUNCH;
    static std::atomic<int> n_cus[64];
    *cus = n_cus[dev].load(std::memory_order_acquire);
    if (*cus == 0) {
        if (hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || *cus < 1) return MPL_E_LAUNCH;
        n_cus[dev].store(*cus, std::memory_order_release);
    }
    return MPL_OK;
}

namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// a failure a kernel of an earlier call reported on the current device fails every later call until it is cleared
inline int earlier_device_failure() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return MPL_E_LAUNCH;
    return device_error_pending(dev) ? MPL_E_DEVICE : MPL_OK;
}

// bump allocator of the workspace carvers: 256-byte aligned pieces from `base` (nullptr: only the size is wanted)
struct WsCarver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align_up(bytes, 256);
        return p;
    }
};

struct StackWs {
    float *qkv, *att, *hid, *stats;
    size_t bytes;
};

StackWs carve_stack_ws(void* base, size_t M, size_t D) {
    WsCarver c{reinterpret_cast<char*>(base)};
    StackWs w;
    w.qkv = c.take<float>(M * 3 * D * sizeof(float));
    w.att = c.take<float>(M * D * sizeof(float));
    w.hid = c.take<float>(M * 2 * D * sizeof(float));
    w.stats = c.take<float>(M * 2 * (size_t)ln_stat_slices((int)D) * sizeof(float));
    w.bytes = c.off;
    return w;
}

std::atomic<int> g_spin_log2{23};    // polls before a wait inside a persistent kernel counts as lost (mpl_x3_spin_limit)

// THE rule for "the packed-operand team kernels (h2_gemm.hip / b1_gemm.hip) take a stack of this shape": a head that tiles the
// 136-column slice with its score matrices in LDS (h2_attention_fusable), a packed layout for every Linear, and D <= 1088: the
// LayerNorm GEMMs (K = D) combine at most 8 slice partials per row, so launch_pack_h2 / launch_pack_b1 fold no LayerNorm into a
// wider operand -- wider multiples of 544 run on the nn.Linear tensors (fp32) or on the shape-general bf16 engine
bool team_stack_shape_ok(int n_tok, int D, int H) {
    return D <= 1088 && h2_attention_fusable(n_tok, D, H) && h2_shape_ok(D, 2 * D);
}

// THE rule for "which bf16 operand layout do the *_w16 fields of a stack of this shape carry" (mpl_bf16_operand_layout): the tuned
// one of mpl_pack_bf16 where the team kernels take the shape (b1_gemm.hip), else the shape-general one of mpl_pack_bf16_any
// (b1_any.hip: any width up to 4096, any head count that divides it, up to 32 tokens per sequence), else none
int bf16_layout(int D, int H, int n_tok) {
    if (D <= 0 || H <= 0 || n_tok <= 0) return MPL_E_INVALID;
    if (team_stack_shape_ok(n_tok, D, H)) return MPL_BF16_TUNED;
    if (n_tok <= 32 && D % H == 0 && D <= 4096 && b1a_operand_bytes(3 * D, D) && b1a_operand_bytes(D, 2 * D)) return MPL_BF16_ANY;
    return MPL_BF16_NONE;
}

// operand_parts of the engine a stack takes: 2 = every block carries fp16x2 operands (h2_gemm.hip, the default fp32 engine), 1 = packed
// bf16 operands in the tuned layout (b1_gemm.hip), 3 = bf16 operands in the shape-general layout (b1_any.hip), 0 = none of them (or the
// shape has no packed layout): the stack then runs on the fp32 matrix instructions.  `parts` = what the blocks carry (1 = *_w16).
constexpr int NP_BF16_ANY = 3;
int engine_parts(int parts, int n_tok, int D, int H) {
    if (parts == 1) {
        const int lay = bf16_layout(D, H, n_tok);
        return lay == MPL_BF16_TUNED ? 1 : (lay == MPL_BF16_ANY ? NP_BF16_ANY : 0);
    }
    return (parts == 2 && team_stack_shape_ok(n_tok, D, H)) ? 2 : 0;
}
// what every scheduled block carries: 1 = the four *_w16 operands, 2 = the four *_h2 operands, 0 = neither, or not all the same
int stack_carried_parts(const mpl_block_weights* blocks, const uint8_t* schedule, int n_apps) {
    int np = 0;
    for (int a = 0; a < n_apps; ++a) {
        const mpl_block_weights& b = blocks[schedule[a]];
        const int bp = (b.qkv_w16 && b.proj_w16 && b.fc1_w16 && b.fc2_w16) ? 1 : ((b.qkv_h2 && b.proj_h2 && b.fc1_h2 && b.fc2_h2) ? 2 : 0);
        if (bp == 0 || (np && bp != np)) return 0;
        np = bp;
    }
    return np;
}

// Workspace of the shape-general bf16 engine (b1_any.hip): x stays fp32 in place; qkv fp32 (the attention reads it), the attention
// output and the GELU output as bf16 rows of leading dimension b1a_ld(width), the LayerNorm slice partials of launch_row_stats
struct AnyWs {
    float* qkv;
    unsigned short *att, *hid;
    float* stats;
    size_t bytes;
};
AnyWs carve_any_ws(void* base, size_t M, size_t D) {
    WsCarver c{reinterpret_cast<char*>(base)};
    AnyWs w;
    w.qkv = c.take<float>(M * 3 * D * sizeof(float));
    w.att = c.take<unsigned short>(M * (size_t)b1a_ld((int)D) * 2);
    w.hid = c.take<unsigned short>(M * (size_t)b1a_ld((int)(2 * D)) * 2);
    w.stats = c.take<float>(M * 2 * (size_t)ln_stat_slices((int)D) * sizeof(float));
    w.bytes = c.off;
    return w;
}

// The block stack on the shape-general bf16 engine: per application a statistics pass, four GEMM launches and the token attention
int block_stack_bf16_any(float* x, int n_seq, int n_tok, int D, int H, const mpl_block_weights* blocks, const uint8_t* schedule,
                         int n_apps, void* ws, size_t ws_bytes, hipStream_t s) {
    const int M = n_seq * n_tok, lda = b1a_ld(D), ldh = b1a_ld(2 * D);
    const float eps = 1e-6f;  // norm_layer = partial(nn.LayerNorm, eps=1e-6), multiview_mpl.py:139
    const AnyWs w = carve_any_ws(ws, (size_t)M, (size_t)D);
    if (!ws || ws_bytes < w.bytes) return MPL_E_WORKSPACE;
    int rc;
    for (int a = 0; a < n_apps; ++a) {
        const mpl_block_weights& b = blocks[schedule[a]];
        // x = x + proj(attn(qkv(norm1(x))))   (Block.forward :84-90)
        if ((rc = launch_row_stats(x, M, D, D, w.stats, s))) return rc;
        if ((rc = launch_b1a_gemm(x, D, nullptr, 0, b.qkv_w16, w.stats, eps, nullptr, w.qkv, 3 * D, M, 3 * D, D, MPL_EPI_BIAS, s))) return rc;
        if ((rc = launch_token_attention_bf16(w.qkv, n_seq, n_tok, D, H, w.att, lda, s))) return rc;
        if ((rc = launch_b1a_gemm(nullptr, 0, w.att, lda, b.proj_w16, nullptr, 0.f, x, x, D, M, D, D, MPL_EPI_BIAS_RESIDUAL, s))) return rc;
        // x = x + fc2(gelu(fc1(norm2(x))))    (Block.forward :91, Mlp.forward :31-37)
        if ((rc = launch_row_stats(x, M, D, D, w.stats, s))) return rc;
        if ((rc = launch_b1a_gemm(x, D, nullptr, 0, b.fc1_w16, w.stats, eps, nullptr, w.hid, ldh, M, 2 * D, D, MPL_EPI_BIAS_GELU, s))) return rc;
        if ((rc = launch_b1a_gemm(nullptr, 0, w.hid, ldh, b.fc2_w16, nullptr, 0.f, x, x, D, M, D, 2 * D, MPL_EPI_BIAS_RESIDUAL, s))) return rc;
    }
    return MPL_OK;
}

// Workspace of the packed-operand engines.  x stays fp32 in place (residual stream, statistics); the attention output and the GELU
// output travel as packed operands of engine np.  fp16x2 (np = 2, h2_gemm.hip): x itself is the A operand of the LayerNorm GEMMs.
// bf16 (np = 1, b1_gemm.hip): x travels to them as the packed bf16 copy x16 that the residual epilogues rewrite.
struct PackedWs {
    unsigned short *x16, *att, *hid;
    float* stats;
    unsigned* counters;
    size_t bytes;
};
PackedWs carve_packed_ws(void* base, size_t M, size_t D, int rpt, int np) {
    WsCarver c{reinterpret_cast<char*>(base)};
    PackedWs w;
    w.x16 = np == 1 ? c.take<unsigned short>(h2_act_bytes((int)M, (int)D, rpt, 1)) : nullptr;
    w.att = c.take<unsigned short>(h2_act_bytes((int)M, (int)D, rpt, np));
    w.hid = c.take<unsigned short>(h2_act_bytes((int)M, (int)(2 * D), rpt, np));
    w.stats = c.take<float>((M + 64) * 2 * (size_t)ln_stat_slices((int)D) * sizeof(float));
    w.counters = c.take<unsigned>((h2_err_index((int)((M + rpt - 1) / rpt)) + 64) * sizeof(unsigned));
    w.bytes = c.off;
    return w;
}

// The block stack on the packed-operand engine NP: the persistent team kernels, or one launch per GEMM (mpl_x3_stack_mode bit 0)
template <int NP>
int block_stack_packed(float* x, int n_seq, int n_tok, int D, int H, const mpl_block_weights* blocks, const uint8_t* schedule,
                       int n_apps, void* ws, size_t ws_bytes, const unsigned** err_ws, hipStream_t s) {
    const int M = n_seq * n_tok, rpt = h2_rows_per_tile(n_tok);
    const float eps = 1e-6f;  // norm_layer = partial(nn.LayerNorm, eps=1e-6), multiview_mpl.py:139
    if (n_apps > MPL_MAX_APPS) return MPL_E_UNSUPPORTED;
    const PackedWs w = carve_packed_ws(ws, (size_t)M, (size_t)D, rpt, NP);
    if (!ws || ws_bytes < w.bytes) return MPL_E_WORKSPACE;
    const int n_tiles = (M + rpt - 1) / rpt;
    if (err_ws) *err_ws = w.counters + h2_err_index(n_tiles);
    int rc;
    const unsigned short* ops[MPL_MAX_APPS * 4];
    for (int a = 0; a < n_apps; ++a) {
        const mpl_block_weights& b = blocks[schedule[a]];
        for (int i = 0; i < 4; ++i) ops[4 * a + i] = NP == 2 ? (&b.qkv_h2)[i] : (&b.qkv_w16)[i];
    }
    // entry of the stack, one launch: LayerNorm slice partials of the incoming rows, zeroed arrival counters + error word; fp16x2:
    // the check that proj / fc2 were packed against the static scales of their producers (mpl_pack_h2_scaled); bf16: the rows as
    // the packed operand x16
    if constexpr (NP == 2) rc = launch_h2_entry(x, M, D, D, w.stats, w.counters, h2_err_index(n_tiles) + 1, ops, n_apps, s);
    else rc = launch_b1_entry(x, M, D, D, rpt, w.x16, w.stats, w.counters, h2_err_index(n_tiles) + 1, s);
    if (rc) return rc;
    const int mode = g_stack_mode.load(), stop = mode >> 8;
    if (!(mode & 1)) {
        if constexpr (NP == 2) return launch_h2_stack(x, M, D, n_tok, H, ops, n_apps, w.att, w.hid, w.stats, w.counters, eps, stop, s);
        else return launch_b1_stack(x, w.x16, M, D, n_tok, H, ops, n_apps, w.att, w.hid, w.stats, w.counters, eps, stop, s);
    }
    // A/B switch (mpl_x3_stack_mode bit 0): the same phases as one launch per GEMM
    for (int a = 0; a < n_apps; ++a) {
        const unsigned short* const* op = ops + 4 * a;
        if constexpr (NP == 2) rc = launch_h2_qkv_attention(x, op[0], w.stats, eps, M, D, n_tok, H, w.att, s);
        else rc = launch_b1_qkv_attention(w.x16, op[0], w.stats, eps, M, D, n_tok, H, w.att, s);
        if (rc) return rc;
        for (int g = 1; g < 4; ++g) {
            if (stop && 4 * a + g >= stop) return MPL_OK;
            if (g == 2) {       // fc1: LayerNorm + GELU -> hid
                if constexpr (NP == 2)
                    rc = launch_h2_gemm(x, nullptr, nullptr, op[g], true, w.stats, eps, nullptr, 0, nullptr, 0, w.hid, nullptr, M, 2 * D, D,
                                        rpt, MPL_EPI_BIAS_GELU, s);
                else rc = launch_b1_gemm(w.x16, op[g], true, w.stats, eps, nullptr, 0, nullptr, 0, w.hid, nullptr, M, 2 * D, D, rpt,
                                         MPL_EPI_BIAS_GELU, s);
            } else {            // proj (A = att, K = D), fc2 (A = hid, K = 2 D): x += ..., its LayerNorm partials (bf16: and x16)
                const unsigned short* A = g == 1 ? w.att : w.hid;
                const int K = g == 1 ? D : 2 * D;
                if constexpr (NP == 2)
                    rc = launch_h2_gemm(nullptr, A, nullptr, op[g], false, nullptr, 0.f, x, D, x, D, nullptr, w.stats, M, D, K, rpt,
                                        MPL_EPI_BIAS_RESIDUAL, s);
                else rc = launch_b1_gemm(A, op[g], false, nullptr, 0.f, x, D, x, D, w.x16, w.stats, M, D, K, rpt, MPL_EPI_BIAS_RESIDUAL, s);
            }
            if (rc) return rc;
        }
    }
    return MPL_OK;
}

thread_local int t_last_form = MPL_E_INVALID;  // MPL_FORM_* of this thread's most recent block-stack launch (mpl_block_stack_last_form)

// THE rule for "the small-batch engine (sm_stack.hip) takes this stack": block_stack_impl launches by it, mpl_block_stack_form
// reports by it.  np = packed operand parts of the blocks (0 none, 2 fp16x2, 1 bf16: an explicit bf16 request keeps its engine);
// raw = every nn.Linear / LayerNorm tensor of every scheduled block is present (the engine reads them in place); cus = compute
// units of the device (every column tile of the widest GEMM needs a resident workgroup of its own: they poll each other's output).
inline bool small_engine_taken(int np, bool allow_small, int M, int D, int n_tok, int H, int n_apps, int n_blocks, bool raw, int cus) {
    const int mode = g_stack_mode.load();
    return (np == 0 || np == 2) && allow_small && !((mode >> 3) & 1) && n_apps <= MPL_MAX_APPS && raw && !(mode & 1) && (mode >> 8) == 0 &&
           sm_stack_ok(M, D, n_tok, H, n_apps, n_blocks, cus);
}

int block_stack_impl(float* x, int n_seq, int n_tok, int D, int H, const mpl_block_weights* blocks,
                     const uint8_t* schedule, int n_apps, void* ws, size_t ws_bytes, const unsigned** err_ws, bool allow_small,
                     hipStream_t s) {
    if (err_ws) *err_ws = nullptr;
    if (!x || n_seq <= 0 || n_tok <= 0 || D <= 0 || H <= 0 || n_apps < 0) return MPL_E_INVALID;
    // row counts are 32-bit in the kernels (byte offsets are 64-bit): refuse what would overflow instead of wrapping
    if ((long long)n_seq * n_tok > (1ll << 30)) return MPL_E_UNSUPPORTED;
    if (n_apps == 0) return MPL_OK;
    // one limit for every engine, the one mpl_block_stack_form_ex answers by (the fp32-MFMA route had none of its own)
    if (n_apps > MPL_MAX_APPS) return MPL_E_UNSUPPORTED;
    // the narrowest GEMM of a block (K = D) decides whether the any-K kernel runs it, and it must take the rows
    if (!ln_gemm_rows_ok((long long)n_seq * n_tok, D, D)) return MPL_E_UNSUPPORTED;
    if (!blocks || !schedule) return MPL_E_INVALID;
    const int carried = stack_carried_parts(blocks, schedule, n_apps);
    const int np0 = carried ? engine_parts(carried, n_tok, D, H) : 0;
    // fp16x2 operands of a shape the team kernels do not take (a head dim 8 stack beyond 14 tokens: h2_attention_fusable) are an
    // fp32 request all the same: the stack runs on the nn.Linear tensors, as mpl_block_stack_form reports (MPL_FORM_UNPACKED)
    const bool ignore_h2 = carried == 2 && np0 == 0;
    // up to 80 token rows (a single frame, a few frames): the whole chip on every GEMM instead of one team of D / 136
    // workgroups (sm_stack.hip) -- for the fp32 engines; an explicit bf16 request keeps its engine
    // (not when the caller asked for batch-invariant bits -- MPL_F_NO_SMALL_STACK --, nor under the A/B switches of the team
    // kernels: one launch per GEMM, stop after n phases).  ONE predicate decides (small_engine_taken): this function launches
    // by it and mpl_block_stack_form reports by it.
    if ((long long)n_seq * n_tok <= sm_stack_max_rows()) {
        int n_blocks = 0;
        bool raw = true;        // the engine reads the nn.Linear tensors in place: a caller that hands over packed operands only
        for (int a = 0; a < n_apps; ++a) {      // (the C ABI allows it) gets the team kernels, not an error
            n_blocks = schedule[a] + 1 > n_blocks ? schedule[a] + 1 : n_blocks;
            const mpl_block_weights& b = blocks[schedule[a]];
            raw = raw && b.ln1_w && b.ln1_b && b.qkv_w && b.qkv_b && b.proj_w && b.proj_b && b.ln2_w && b.ln2_b && b.fc1_w && b.fc1_b &&
                  b.fc2_w && b.fc2_b;
        }
        int cus = 0;
        if (device_cu_count(&cus) != MPL_OK) return MPL_E_LAUNCH;
        if (small_engine_taken(np0, allow_small, n_seq * n_tok, D, n_tok, H, n_apps, n_blocks, raw, cus)) {
            const int rc = launch_sm_stack(x, n_seq, n_tok, D, H, blocks, schedule, n_apps, ws, ws_bytes, err_ws, g_spin_log2.load(), s);
            if (rc != MPL_E_UNSUPPORTED) {               // (UNSUPPORTED: the occupancy query refused one workgroup per CU -- the team kernels below)
                if (rc == MPL_OK) t_last_form = MPL_FORM_SMALL;
                return rc;
            }
            if (err_ws) *err_ws = nullptr;
        }
    }
    if (np0 == NP_BF16_ANY) {
        const int rc = block_stack_bf16_any(x, n_seq, n_tok, D, H, blocks, schedule, n_apps, ws, ws_bytes, s);
        if (rc == MPL_OK) t_last_form = MPL_FORM_BF16_ANY;
        return rc;
    }
    if (const int np = np0) {
        const int rc = np == 2 ? block_stack_packed<2>(x, n_seq, n_tok, D, H, blocks, schedule, n_apps, ws, ws_bytes, err_ws, s)
                               : block_stack_packed<1>(x, n_seq, n_tok, D, H, blocks, schedule, n_apps, ws, ws_bytes, err_ws, s);
        if (rc == MPL_OK) {
            int cus = 0;
            t_last_form = (g_stack_mode.load() & 1) ? (int)MPL_FORM_PER_GEMM
                          : (device_cu_count(&cus) == MPL_OK ? h2_stack_form_code(n_seq * n_tok, D, n_tok, np, cus) : (int)MPL_E_LAUNCH);
        }
        return rc;
    }
    t_last_form = MPL_FORM_UNPACKED;
    const int M = n_seq * n_tok;
    const StackWs w = carve_stack_ws(ws, (size_t)M, (size_t)D);
    if (!ws || ws_bytes < w.bytes) return MPL_E_WORKSPACE;
    const float eps = 1e-6f;  // norm_layer = partial(nn.LayerNorm, eps=1e-6), multiview_mpl.py:139
    int rc;
    // LayerNorm statistics are produced by whoever writes x: a stand-alone pass for the incoming x, then the
    // epilogues of proj (-> norm2) and fc2 (-> norm1 of the next application).
    float* st_out = (D % 136 == 0 && D % 32 == 0) ? w.stats : nullptr;      // (a width the tuned GEMMs take: launch_ln_gemm)
    bool have_stats = false;
    // qkv projection and attention run as one kernel when a 64-row tile holds whole sequences and a 136-column
    // slice whole heads (V in {1,2,4,8,16,32,64}; hd in {68,136}); otherwise as two kernels through `qkv`
    const bool fusable = qkv_attention_fusable(n_tok, D, H);
    // D = 32 blocks (keypoint-token FPT) that carry the operand of mpl_d32_pack in qkv_w3: everything but the attention is
    // row-local and runs as two launches from split fp16 operands (d32_blocks.hip: d32_qkv_kernel, d32_mlp_kernel)
    bool d32 = D == 32;
    for (int a = 0; a < n_apps && d32; ++a) {
        const mpl_block_weights& b = blocks[schedule[a]];
        d32 = b.qkv_w3 && !b.proj_w3 && !b.fc1_w3 && !b.fc2_w3 && !b.qkv_w16 && !b.qkv_h2;
    }
    if (d32) {
        for (int a = 0; a < n_apps; ++a) {
            const mpl_block_weights& b = blocks[schedule[a]];
            if ((rc = launch_d32_qkv(x, M, b.qkv_w3, w.qkv, s))) return rc;
            if ((rc = launch_token_attention(w.qkv, n_seq, n_tok, D, H, w.att, s))) return rc;
            if ((rc = launch_d32_mlp(x, w.att, M, b.qkv_w3, s))) return rc;
        }
        return MPL_OK;
    }
    // every scheduled block is looked at before the first launch: a refusal leaves x untouched.  Packed operands (fp16x2 / bf16)
    // take the routes above and cannot be used here, except fp16x2 operands without an engine (ignore_h2), which are not read --
    // the nn.Linear tensors must then be there
    for (int a = 0; a < n_apps; ++a) {
        const mpl_block_weights& b = blocks[schedule[a]];
        if (b.qkv_w3 || b.proj_w3 || b.fc1_w3 || b.fc2_w3 || b.qkv_w16 || b.proj_w16 || b.fc1_w16 || b.fc2_w16 ||
            (!ignore_h2 && (b.qkv_h2 || b.proj_h2 || b.fc1_h2 || b.fc2_h2)))
            return MPL_E_UNSUPPORTED;
        if (ignore_h2 && !(b.ln1_w && b.ln1_b && b.qkv_w && b.qkv_b && b.proj_w && b.proj_b && b.ln2_w && b.ln2_b && b.fc1_w && b.fc1_b &&
                           b.fc2_w && b.fc2_b))
            return MPL_E_UNSUPPORTED;
    }
    for (int a = 0; a < n_apps; ++a) {
        const mpl_block_weights& b = blocks[schedule[a]];
        const bool fused_att = fusable;
        // x = x + proj(attn(qkv(norm1(x))))   (Block.forward :84-90)
        if (!have_stats && (rc = launch_row_stats(x, M, D, D, w.stats, s))) return rc;
        if (fused_att) {
            rc = launch_ln_qkv_attention(x, M, D, w.stats, b.ln1_w, b.ln1_b, eps, b.qkv_w, b.qkv_b, n_tok, H, w.att, s);
            if (rc) return rc;
        } else {
            rc = launch_ln_gemm(x, D, w.stats, b.ln1_w, b.ln1_b, eps, b.qkv_w, b.qkv_b, nullptr, 0, w.qkv, 3 * D, M,
                                3 * D, D, MPL_EPI_BIAS, nullptr, s);
            if (rc) return rc;
            if ((rc = launch_token_attention(w.qkv, n_seq, n_tok, D, H, w.att, s))) return rc;
        }
        rc = launch_ln_gemm(w.att, D, nullptr, nullptr, nullptr, 0.f, b.proj_w, b.proj_b, x, D, x, D, M, D, D,
                            MPL_EPI_BIAS_RESIDUAL, st_out, s);
        if (rc) return rc;
        // x = x + fc2(gelu(fc1(norm2(x))))    (Block.forward :91, Mlp.forward :31-37)
        if (!st_out && (rc = launch_row_stats(x, M, D, D, w.stats, s))) return rc;
        rc = launch_ln_gemm(x, D, w.stats, b.ln2_w, b.ln2_b, eps, b.fc1_w, b.fc1_b, nullptr, 0, w.hid, 2 * D, M,
                            2 * D, D, MPL_EPI_BIAS_GELU, nullptr, s);
        if (rc) return rc;
        rc = launch_ln_gemm(w.hid, 2 * D, nullptr, nullptr, nullptr, 0.f, b.fc2_w, b.fc2_b, x, D, x, D, M, D,
                            2 * D, MPL_EPI_BIAS_RESIDUAL, st_out, s);
        if (rc) return rc;
        have_stats = st_out != nullptr;
    }
    return MPL_OK;
}

// hipGetLastError() is per-thread state shared with the caller: a benign failure inside the caller's own HIP use (e.g.
// torch probing a host pointer) would otherwise be reported by the first launch check of this library.
inline void clear_stale_hip_error() { (void)hipGetLastError(); }

// either engine may run the stack (the binding decides by the operands it supplies): size for the larger layout
size_t stack_ws_bytes(size_t M, size_t D, int n_tok) {
    size_t b = carve_stack_ws(nullptr, M, D).bytes;
    if (M <= (size_t)sm_stack_max_rows()) {
        const size_t bs = sm_stack_ws_bytes((int)M, (int)D);
        b = bs > b ? bs : b;
    }
    const int rpt = h2_rows_per_tile(n_tok);
    if (rpt > 0 && n_tok <= 32 && h2_shape_ok((int)D, (int)(2 * D))) {
        const size_t b2 = carve_packed_ws(nullptr, M, D, rpt, 2).bytes;
        b = b2 > b ? b2 : b;
        const size_t b1 = carve_packed_ws(nullptr, M, D, rpt, 1).bytes;
        b = b1 > b ? b1 : b;
    }
    if (n_tok <= 32 && D <= 4096) {
        const size_t ba = carve_any_ws(nullptr, M, D).bytes;
        b = ba > b ? ba : b;
    }
    return b;
}

int check_cfg(const mpl_config* cfg) {
    if (!cfg) return MPL_E_INVALID;
    if (cfg->num_views < 1 || cfg->num_views > MPL_MAX_VIEWS || cfg->depth < 0 || cfg->depth > 60) return MPL_E_INVALID;
    return MPL_OK;
}

// the joints x views token grid of a keypoint-token FPT: the attention kernels that take it (launch_token_attention)
bool kptok_attention_ok(int n_tok, int hd) { return token_attention_ok(n_tok, hd); }

}  // namespace

extern "C" {

int mpl_profile_start(void) {
    std::lock_guard<std::mutex> g(g_prof_mu);
    g_prof.clear();
    g_prof_on.store(true);
    return MPL_OK;
}

int mpl_profile_stop(float* kind_ms, int* kind_launches, int n_kinds) {
    g_prof_on.store(false);
    std::lock_guard<std::mutex> g(g_prof_mu);
    if (!kind_ms || !kind_launches || n_kinds < MPL_K_COUNT) return MPL_E_INVALID;
    for (int k = 0; k < n_kinds; ++k) {
        kind_ms[k] = 0.f;
        kind_launches[k] = 0;
    }
    int rc = MPL_OK;
    for (auto& r : g_prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) rc = MPL_E_LAUNCH;
        kind_ms[r.kind] += ms;
        kind_launches[r.kind] += 1;
        hipEventDestroy(r.e0);
        hipEventDestroy(r.e1);
    }
    g_prof.clear();
    return rc;
}

int mpl_hip_abi_version(void) { return MPL_HIP_ABI_VERSION; }

const char* mpl_hip_error_string(int code) {
    switch (code) {
        case MPL_OK: return "ok";
        case MPL_E_INVALID: return "invalid argument or shape";
        case MPL_E_UNSUPPORTED: return "configuration not supported by the HIP path";
        case MPL_E_WORKSPACE: return "workspace missing or too small";
        case MPL_E_LAUNCH: return "HIP runtime error at kernel launch";
        case MPL_E_DEVICE:
            return "an earlier forward on this device failed on the device and its poses are NaN (mpl_device_error() bits: 1 = a "
                   "workgroup of the persistent block-stack kernel lost a hand-off -- the GPU was shared with other work for "
                   "longer than the wait bound -- or proj / fc2 operands were not packed against their producers' scales "
                   "(mpl_pack_h2_scaled skipped); 2 = confidence_as_attention_uncertainty_weight with confidences so large that "
                   "the weighted attention output left the fp16 window of the split operands: run that model with "
                   "set_matmul_precision('fp32_mfma'), the native-fp32 engine has no window); clear with mpl_device_error_clear()";
        default: return "unknown error";
    }
}

int mpl_config_supported(const mpl_config* cfg) {
    if (!cfg) return MPL_E_INVALID;
    const unsigned f = cfg->flags;
    const int J = cfg->num_joints, d = cfg->dim, H = cfg->heads, V = cfg->num_views;
    if (J < 1 || J > 64 || d < 1 || d > 128 || H < 1 || d % H) return MPL_E_UNSUPPORTED;
    if (V < 1 || V > MPL_MAX_VIEWS || cfg->depth < 0 || cfg->depth > 60) return MPL_E_UNSUPPORTED;
    if ((f & MPL_F_CONF_ATTN_W) && !(f & MPL_F_NO_SPT) && cfg->depth > 31) return MPL_E_UNSUPPORTED;    // SPT schedule length
    if ((long long)J * d * ((f & MPL_F_RAYS_TOKEN) ? 2 : 1) > 4096) return MPL_E_UNSUPPORTED;
    if ((f & MPL_F_POS3D_TO_RAYS) && (!(f & MPL_F_RAYS_TOKEN) || (f & MPL_F_POS3D_SPATIAL))) return MPL_E_UNSUPPORTED;
    if ((f & MPL_F_KPTOK) && !(f & MPL_F_NO_FPT) && cfg->depth > 0) {
        if ((f & MPL_F_RAYS_TOKEN) || !kptok_attention_ok(J * V, d / H)) return MPL_E_UNSUPPORTED;
    }
    return MPL_OK;
}

int mpl_fpt_width(const mpl_config* cfg) {
    if (!cfg) return MPL_E_INVALID;
    return cfg->num_joints * cfg->dim * ((cfg->flags & MPL_F_RAYS_TOKEN) ? 2 : 1);
}

size_t mpl_block_stack_workspace_bytes(int n_seq, int n_tok, int dim) {
    return stack_ws_bytes((size_t)n_seq * n_tok, (size_t)dim, n_tok);
}

size_t mpl_forward_workspace_bytes(const mpl_config* cfg, int batch) {
    if (!cfg || batch <= 0) return 0;
    const size_t M = (size_t)batch * cfg->num_views, D = (size_t)mpl_fpt_width(cfg);
    // joints x views token grid (:496-497): the same xs memory seen as (B, V*J, d)
    const bool kp = (cfg->flags & MPL_F_KPTOK) != 0;
    const size_t Ms = kp ? M * cfg->num_joints : M, Ds = kp ? (size_t)cfg->dim : D;
    return align_up(M * D * sizeof(float), 256) + stack_ws_bytes(Ms, Ds, kp ? cfg->num_views * cfg->num_joints : cfg->num_views);
}

int mpl_spt_tokens(const mpl_config* cfg, const mpl_weights* w, const mpl_inputs* in, float* xs, void* stream) {
    clear_stale_hip_error();
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if ((rc = mpl_config_supported(cfg))) return rc;
    if (!w || !in || !xs) return MPL_E_INVALID;
    return launch_spt(cfg, w, in, xs, w->spt_packed != 0, (hipStream_t)stream);
}

int mpl_block_stack_ex(float* x, int n_seq, int n_tok, int dim, int heads, const mpl_block_weights* blocks,
                       const uint8_t* schedule, int n_apps, void* workspace, size_t workspace_bytes, unsigned flags, void* stream) {
    clear_stale_hip_error();
    if (int rc = earlier_device_failure()) return rc;
    return block_stack_impl(x, n_seq, n_tok, dim, heads, blocks, schedule, n_apps, workspace, workspace_bytes, nullptr,
                            (flags & MPL_F_NO_SMALL_STACK) == 0, (hipStream_t)stream);
}

int mpl_block_stack(float* x, int n_seq, int n_tok, int dim, int heads, const mpl_block_weights* blocks,
                    const uint8_t* schedule, int n_apps, void* workspace, size_t workspace_bytes, void* stream) {
    return mpl_block_stack_ex(x, n_seq, n_tok, dim, heads, blocks, schedule, n_apps, workspace, workspace_bytes, 0u, stream);
}

int mpl_ln_linear(const float* x, int M, int K, const float* ln_w, const float* ln_b, float eps, const float* W,
                  const float* bias, int N, int epilogue, const float* residual, float* y, float* stats,
                  void* stream) {
    clear_stale_hip_error();
    if (!x || !W || !bias || !y) return MPL_E_INVALID;
    if (M > 0 && K > 0 && !ln_gemm_rows_ok(M, K, K)) return MPL_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (ln_w) {
        if (!stats) return MPL_E_INVALID;
        int rc = launch_row_stats(x, M, K, K, stats, s);
        if (rc) return rc;
    }
    return launch_ln_gemm(x, K, stats, ln_w, ln_b, eps, W, bias, residual, N, y, N, M, N, K, epilogue, nullptr, s);
}

size_t mpl_spt_pack_bytes(void) { return spt_pack_bytes(); }

int mpl_spt_pack(const mpl_block_weights* block, uint16_t* dst, void* stream) {
    clear_stale_hip_error();
    return launch_spt_pack(block, dst, 1, (hipStream_t)stream);
}

int mpl_d32_pack(const mpl_block_weights* block, uint16_t* dst, void* stream) {
    clear_stale_hip_error();
    return launch_spt_pack(block, dst, 0, (hipStream_t)stream);
}

size_t mpl_pack_bf16_bytes(int N, int K) { return h2_operand_bytes(N, K, 1); }

int mpl_pack_bf16(const float* W, const float* bias, const float* ln_w, const float* ln_b, int N, int K, uint16_t* dst, void* stream) {
    clear_stale_hip_error();
    if (mpl_pack_bf16_bytes(N, K) == 0) return MPL_E_INVALID;
    return launch_pack_b1(W, N, K, ln_w, ln_b, bias, dst, (hipStream_t)stream);
}

int mpl_bf16_operand_layout(int dim, int heads, int n_tok) { return bf16_layout(dim, heads, n_tok); }
int mpl_team_stack_shape(int dim, int heads, int n_tok) {
    if (dim <= 0 || heads <= 0 || n_tok <= 0) return MPL_E_INVALID;
    return team_stack_shape_ok(n_tok, dim, heads) ? 1 : 0;
}

size_t mpl_pack_bf16_any_bytes(int N, int K) { return b1a_operand_bytes(N, K); }

int mpl_pack_bf16_any(const float* W, const float* bias, const float* ln_w, const float* ln_b, int N, int K, uint16_t* dst, void* stream) {
    clear_stale_hip_error();
    if (mpl_pack_bf16_any_bytes(N, K) == 0) return MPL_E_INVALID;
    return launch_pack_b1a(W, N, K, ln_w, ln_b, bias, dst, (hipStream_t)stream);
}

size_t mpl_ln_linear_bf16_any_workspace_bytes(int M, int K) {
    if (M <= 0 || K <= 0 || K > 8192) return 0;
    return (size_t)M * b1a_ld(K) * 2;
}

int mpl_ln_linear_bf16_any(const float* x, int M, int K, int has_ln, float eps, const uint16_t* W16, int N, int epilogue,
                           const float* residual, void* y, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    clear_stale_hip_error();
    if (!x || !W16 || !y || M <= 0 || b1a_operand_bytes(N, K) == 0) return MPL_E_INVALID;
    if (!ln_gemm_rows_ok(M, K, K)) return MPL_E_UNSUPPORTED;        // the row envelope of the block stack (block_stack_impl)
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (has_ln) {
        if (!stats) return MPL_E_INVALID;
        if (epilogue != MPL_EPI_BIAS && epilogue != MPL_EPI_BIAS_GELU) return MPL_E_UNSUPPORTED;
        if ((rc = launch_row_stats(x, M, K, K, stats, s))) return rc;
        return launch_b1a_gemm(x, K, nullptr, 0, W16, stats, eps, nullptr, y, N, M, N, K, epilogue, s);
    }
    if (epilogue != MPL_EPI_BIAS_RESIDUAL || !residual) return MPL_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < mpl_ln_linear_bf16_any_workspace_bytes(M, K)) return MPL_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return MPL_E_INVALID;
    unsigned short* a16 = reinterpret_cast<unsigned short*>(workspace);
    if ((rc = launch_b1a_rows(x, M, K, a16, s))) return rc;
    return launch_b1a_gemm(nullptr, 0, a16, b1a_ld(K), W16, nullptr, 0.f, residual, y, N, M, N, K, epilogue, s);
}

size_t mpl_pack_h2_bytes(int N, int K) { return h2_operand_bytes(N, K); }

int mpl_pack_h2(const float* W, const float* bias, const float* ln_w, const float* ln_b, int N, int K, uint16_t* dst, void* stream) {
    clear_stale_hip_error();
    if (mpl_pack_h2_bytes(N, K) == 0) return MPL_E_INVALID;
    return launch_pack_h2(W, N, K, ln_w, ln_b, bias, nullptr, dst, (hipStream_t)stream);
}

int mpl_pack_h2_scaled(const float* W, const float* bias, const float* in_scale, int N, int K, uint16_t* dst, void* stream) {
    clear_stale_hip_error();
    if (mpl_pack_h2_bytes(N, K) == 0 || !in_scale) return MPL_E_INVALID;
    return launch_pack_h2(W, N, K, nullptr, nullptr, bias, in_scale, dst, (hipStream_t)stream);
}

const float* mpl_pack_h2_out_scale(const uint16_t* operand, int N, int K) { return h2_out_scale(operand, N, K); }

size_t mpl_ln_linear_h2_workspace_bytes(int M, int K) {
    const size_t a = h2_act_bytes(M, K, 64);
    return a ? a + 256 : 0;
}

int mpl_ln_linear_h2(const float* x, int M, int K, int has_ln, float eps, const uint16_t* W2, int N, int epilogue,
                     const float* residual, float* y, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    clear_stale_hip_error();
    if (!x || !W2 || !y || h2_operand_bytes(N, K) == 0 || M <= 0) return MPL_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (has_ln) {
        if (!stats) return MPL_E_INVALID;
        if ((rc = launch_row_stats(x, M, K, K, stats, s))) return rc;
        return launch_h2_gemm(x, nullptr, nullptr, W2, true, stats, eps, residual, N, y, N, nullptr, nullptr, M, N, K, 64, epilogue, s);
    }
    const size_t need = mpl_ln_linear_h2_workspace_bytes(M, K);
    if (!workspace || workspace_bytes < need) return MPL_E_WORKSPACE;
    float* sc = reinterpret_cast<float*>(workspace);
    unsigned short* a2 = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(workspace) + 256);
    if ((rc = launch_h2_pack_rows(x, M, K, K, 64, a2, sc, s))) return rc;
    return launch_h2_gemm(nullptr, a2, sc + 2, W2, false, nullptr, 0.f, residual, N, y, N, nullptr, nullptr, M, N, K, 64, epilogue, s);
}

int mpl_block_stack_form_ex(int n_seq, int n_tok, int D, int heads, int n_apps, int n_blocks, int raw_tensors, int operand_parts,
                            unsigned flags) {
    if (n_seq <= 0 || n_tok <= 0 || D <= 0 || heads <= 0 || n_apps <= 0 || n_apps > MPL_MAX_APPS || n_blocks <= 0 || n_blocks > n_apps ||
        operand_parts < 0 || operand_parts > 2)
        return MPL_E_INVALID;
    if ((long long)n_seq * n_tok > (1ll << 30)) return MPL_E_UNSUPPORTED;
    const int M = n_seq * n_tok;
    // the same questions, in the same order, as block_stack_impl asks -- through the same predicates
    const int np = engine_parts(operand_parts, n_tok, D, heads);
    int cus = 0;
    if (device_cu_count(&cus) != MPL_OK) return MPL_E_LAUNCH;
    if (M <= sm_stack_max_rows() && small_engine_taken(np, !(flags & MPL_F_NO_SMALL_STACK), M, D, n_tok, heads, n_apps, n_blocks, raw_tensors != 0, cus))
        return MPL_FORM_SMALL;
    if (np == 0) return MPL_FORM_UNPACKED;
    if (np == NP_BF16_ANY) return MPL_FORM_BF16_ANY;
    if (g_stack_mode.load() & 1) return MPL_FORM_PER_GEMM;
    return h2_stack_form_code(M, D, n_tok, np, cus);
}

// the reference's schedule (every block once, the last one twice: multiview_mpl.py:420-423) with the nn.Linear tensors present
int mpl_block_stack_form(int n_seq, int n_tok, int D, int heads, int n_apps, int operand_parts, unsigned flags) {
    return mpl_block_stack_form_ex(n_seq, n_tok, D, heads, n_apps, n_apps > 1 ? n_apps - 1 : 1, 1, operand_parts, flags);
}

int mpl_block_stack_last_form(void) { return t_last_form; }

int mpl_spt_form(const mpl_config* cfg, int batch, int use_packed, int n_cus, int* seq_per_wg) {
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if ((rc = mpl_config_supported(cfg))) return rc;
    if (batch <= 0) return MPL_E_INVALID;
    if (n_cus <= 0 && (rc = device_cu_count(&n_cus))) return rc;
    int spw = 0;
    rc = spt_form(cfg, batch, use_packed, n_cus, &spw);
    if (rc >= 0 && seq_per_wg) *seq_per_wg = spw;
    return rc;
}

int mpl_x3_stack_mode(int one_launch_per_gemm) {
    g_stack_mode.store(one_launch_per_gemm);      // the bits: common.hpp stack_mode()
    return MPL_OK;
}

int mpl_device_error(int device) {
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return 0;
    return device_error_pending(device);
}

int mpl_device_error_clear(int device) {
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return MPL_E_LAUNCH;
    device_error_clear(device);
    return MPL_OK;
}

int mpl_x3_spin_limit(int log2_polls) {
    if ((log2_polls & 0xff) < 1 || (log2_polls & 0xff) > 30 || log2_polls < 0) return MPL_E_INVALID;
    // the fault injection (bits 8..) is compiled into the product library but inert unless the process opted in
    // (MPL_FAULT_INJECT=1 in the environment at the FIRST call of this function), and it is ONE-SHOT: the first stack launch that
    // consumes it clears it, so a test that dies between set and reset cannot leave the process deserting workgroups
    static const bool inject_ok = getenv("MPL_FAULT_INJECT") != nullptr && atoi(getenv("MPL_FAULT_INJECT")) != 0;
    if ((log2_polls >> 8) != 0 && !inject_ok) return MPL_E_UNSUPPORTED;
    g_spin_log2.store(log2_polls & 0xff);
    h2_set_spin_log2(log2_polls & 0xff);
    set_fault_injection(log2_polls >> 8);
    return MPL_OK;
}

int mpl_x3_debug_buffer(void* device_buffer) {
    h2_set_debug_buffer(reinterpret_cast<unsigned long long*>(device_buffer));
    return MPL_OK;
}

int mpl_token_attention(const float* qkv, int n_seq, int n_tok, int dim, int heads, float* out, void* stream) {
    clear_stale_hip_error();
    if (!qkv || !out) return MPL_E_INVALID;
    return launch_token_attention(qkv, n_seq, n_tok, dim, heads, out, (hipStream_t)stream);
}

int mpl_fuse_head(const mpl_config* cfg, const mpl_weights* w, const float* x, int batch, float* out, void* stream) {
    clear_stale_hip_error();
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!w || !x || !out) return MPL_E_INVALID;
    return launch_fuse_head(cfg, w, x, batch, out, nullptr, nullptr, (hipStream_t)stream);
}

int mpl_view_fuse(const mpl_config* cfg, const mpl_weights* w, const float* x, int batch, float* y, void* stream) {
    clear_stale_hip_error();
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!w || !x || !y) return MPL_E_INVALID;
    return launch_fuse_head(cfg, w, x, batch, nullptr, y, nullptr, (hipStream_t)stream);
}

int mpl_view_norm(const mpl_config* cfg, const mpl_weights* w, const float* x, int batch, float* xn, void* stream) {
    clear_stale_hip_error();
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (!w || !x || !xn || batch <= 0) return MPL_E_INVALID;
    return launch_view_norm(cfg, w, x, batch, xn, (hipStream_t)stream);
}

int mpl_layernorm(const float* x, int M, int K, const float* gamma, const float* beta, float eps, float* y,
                  void* stream) {
    clear_stale_hip_error();
    if (!x || !gamma || !beta || !y) return MPL_E_INVALID;
    return launch_layernorm_rows(x, M, K, K, gamma, beta, eps, y, K, (hipStream_t)stream);
}

int mpl_linear(const float* xa, int Ka, const float* xb, int Kb, int M, const float* W, const float* bias, int N,
               const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, float bn_eps, int relu,
               float* y, void* stream) {
    clear_stale_hip_error();
    return launch_linear_act(xa, Ka, Ka, xb, Kb, Kb, M, W, Ka + Kb, bias, N, bn_w, bn_b, bn_mean, bn_var, bn_eps, relu, y, N,
                             (hipStream_t)stream);
}

int mpl_prepare_inputs(const float* joints_px, const float* conf, const double* cams_dev, int batch, int views, int joints,
                       float img_w, float img_h, int normalize_inputs, int normalize_cameras, float* const* poses,
                       float* const* rays, float* const* centers, void* stream) {
    clear_stale_hip_error();
    return launch_prepare_inputs(joints_px, conf, cams_dev, nullptr, batch, views, joints, img_w, img_h, normalize_inputs,
                                 normalize_cameras, poses, rays, centers, (hipStream_t)stream);
}

int mpl_prepare_inputs_ex(const float* joints_px, const float* conf, const double* cams_dev, const double* dist_dev, int batch,
                          int views, int joints, float img_w, float img_h, int normalize_inputs, int normalize_cameras,
                          float* const* poses, float* const* rays, float* const* centers, void* stream) {
    clear_stale_hip_error();
    return launch_prepare_inputs(joints_px, conf, cams_dev, dist_dev, batch, views, joints, img_w, img_h, normalize_inputs,
                                 normalize_cameras, poses, rays, centers, (hipStream_t)stream);
}

int mpl_undistort_points(const float* pixels, const double* cams_dev, const double* dist_dev, int batch, int views, int joints,
                         int direction, float* out_pixels, unsigned char* out_valid, void* stream) {
    clear_stale_hip_error();
    return launch_undistort_points(pixels, cams_dev, dist_dev, batch, views, joints, direction, out_pixels, out_valid,
                                   (hipStream_t)stream);
}

int mpl_decode_heatmaps(const void* const* heatmaps, int dtype, long long batch_stride, int batch, int views, int joints, int height,
                        int width, int post_process, const float* center, const float* scale, float* pixels, float* conf,
                        float* coords, const double* cams_dev, float img_w, float img_h, int normalize_inputs, int normalize_cameras,
                        float* const* poses, float* const* rays, float* const* centers, void* stream) {
    clear_stale_hip_error();
    return launch_decode_heatmaps(heatmaps, dtype, batch_stride, batch, views, joints, height, width, post_process, center, scale,
                                  pixels, conf, coords, cams_dev, img_w, img_h, normalize_inputs, normalize_cameras, poses, rays,
                                  centers, (hipStream_t)stream);
}

int mpl_decode_heatmaps_ex(const void* const* heatmaps, int dtype, long long batch_stride, int batch, int views, int joints, int height,
                           int width, int post_process, const float* center, const float* scale, float* pixels, float* conf,
                           float* coords, const double* cams_dev, float img_w, float img_h, int normalize_inputs, int normalize_cameras,
                           float* const* poses, float* const* rays, float* const* centers, int refine, int radius, double threshold,
                           void* stream) {
    clear_stale_hip_error();
    return launch_decode_heatmaps_ex(heatmaps, dtype, batch_stride, batch, views, joints, height, width, post_process, center, scale,
                                     pixels, conf, coords, cams_dev, img_w, img_h, normalize_inputs, normalize_cameras, poses, rays,
                                     centers, refine, radius, threshold, (hipStream_t)stream);
}

int mpl_render_heatmaps(void* const* heatmaps, int dtype, long long batch_stride, int batch, int views, int joints, int height, int width,
                        const float* pixels, const float* conf, const float* center, const float* scale, double stride_x,
                        double stride_y, int mode, double sigma, double noise_level, uint64_t noise_key, long long first_index,
                        float* weight, float* cells, void* stream) {
    clear_stale_hip_error();
    return launch_render_heatmaps(heatmaps, dtype, batch_stride, batch, views, joints, height, width, pixels, conf, center, scale,
                                  stride_x, stride_y, mode, sigma, noise_level, noise_key, first_index, weight, cells,
                                  (hipStream_t)stream);
}

size_t mpl_rpsm_workspace_bytes(int batch, int joints, int first_nbins) { return rpsm_workspace_bytes(batch, joints, first_nbins); }

int mpl_rpsm(const void* const* heatmaps, int dtype, long long batch_stride, int batch, int views, int joints, int height, int width,
             const float* center, const float* scale, const double* cams_dev, const double* dist_dev, double img_w, double img_h,
             const float* root_center, const float* limb, long long limb_stride, const int* parents, int first_nbins, int recur_nbins,
             int recur_depth, double grid_size, double tolerance, void* workspace, size_t workspace_bytes, float* poses, int32_t* bins,
             double* energy, int stages, void* stream) {
    clear_stale_hip_error();
    return launch_rpsm(heatmaps, dtype, batch_stride, batch, views, joints, height, width, center, scale, cams_dev, dist_dev, img_w,
                       img_h, root_center, limb, limb_stride, parents, first_nbins, recur_nbins, recur_depth, grid_size, tolerance,
                       workspace, workspace_bytes, poses, bins, energy, stages, (hipStream_t)stream);
}

int mpl_synthesize_views(const float* poses3d, const double* cams_dev, const mpl_synth_options* opt, const float* conf,
                         const float* rotation_deg, const float* translation, const float* noise, const float* missing_u, int batch,
                         int views, int joints, float* const* poses, float* const* rays, float* const* centers, float* target,
                         float* pixels, float* pixels_clean, float* depth, void* stream) {
    clear_stale_hip_error();
    return launch_synthesize_views(poses3d, cams_dev, nullptr, opt, conf, rotation_deg, translation, noise, missing_u, batch, views,
                                   joints, poses, rays, centers, target, pixels, pixels_clean, depth, (hipStream_t)stream);
}

int mpl_synthesize_views_ex(const float* poses3d, const double* cams_dev, const double* dist_dev, const mpl_synth_options* opt,
                            const float* conf, const float* rotation_deg, const float* translation, const float* noise,
                            const float* missing_u, int batch, int views, int joints, float* const* poses, float* const* rays,
                            float* const* centers, float* target, float* pixels, float* pixels_clean, float* depth, void* stream) {
    clear_stale_hip_error();
    return launch_synthesize_views(poses3d, cams_dev, dist_dev, opt, conf, rotation_deg, translation, noise, missing_u, batch, views,
                                   joints, poses, rays, centers, target, pixels, pixels_clean, depth, (hipStream_t)stream);
}

int mpl_triangulate_rays(const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int batch,
                         int views, int joints, float* out_points, float* out_residual, void* stream) {
    clear_stale_hip_error();
    return launch_triangulate_rays(rays, centers, conf, conf_stride, batch, views, joints, out_points, out_residual, (hipStream_t)stream);
}

int mpl_epipolar_errors(const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int batch,
                        int views, int joints, float* out_err, const float* weight_in, float threshold, float* weight_out,
                        void* stream) {
    clear_stale_hip_error();
    return launch_epipolar_errors(rays, centers, conf, conf_stride, batch, views, joints, out_err, weight_in, threshold, weight_out,
                                  (hipStream_t)stream);
}

int mpl_triangulate_robust(const float* const* rays, const float* const* centers, const float* const* conf, int conf_stride, int batch,
                           int views, int joints, double threshold, double conf_threshold, int min_inliers, float* out_points,
                           float* out_residual, float* out_inliers, void* stream) {
    clear_stale_hip_error();
    return launch_triangulate_robust(rays, centers, conf, conf_stride, batch, views, joints, threshold, conf_threshold, min_inliers,
                                     out_points, out_residual, out_inliers, (hipStream_t)stream);
}

int mpl_refine_points(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                      int batch, int views, int joints, double huber, int max_iterations, double step_tolerance, float* out_points,
                      float* out_error, float* out_errors, int* out_iterations, unsigned char* out_status, void* stream) {
    clear_stale_hip_error();
    return launch_refine_points(points, pixels, conf, cams_dev, dist_dev, batch, views, joints, huber, max_iterations, step_tolerance,
                                out_points, out_error, out_errors, out_iterations, out_status, (hipStream_t)stream);
}

int mpl_refine_cameras(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                       int batch, int views, int joints, double huber, int max_iterations, double step_tolerance, unsigned fixed_mask,
                       double* out_cams, double* out_error, double* out_cost0, double* out_cost, int* out_used, int* out_iterations,
                       unsigned char* out_status, void* stream) {
    clear_stale_hip_error();
    return launch_refine_cameras(points, pixels, conf, cams_dev, dist_dev, batch, views, joints, huber, max_iterations, step_tolerance,
                                 fixed_mask, out_cams, out_error, out_cost0, out_cost, out_used, out_iterations, out_status,
                                 (hipStream_t)stream);
}

int mpl_refine_poses(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                     const float* limb, long long limb_stride, const int* parents, int batch, int views, int joints, double huber,
                     double bone_weight, int max_iterations, double step_tolerance, float* out_points, float* out_error,
                     float* out_bone_error, double* out_cost0, double* out_cost, int* out_iterations, unsigned char* out_status,
                     void* stream) {
    clear_stale_hip_error();
    return launch_refine_poses(points, pixels, conf, cams_dev, dist_dev, limb, limb_stride, parents, batch, views, joints, huber,
                               bone_weight, max_iterations, step_tolerance, out_points, out_error, out_bone_error, out_cost0, out_cost,
                               out_iterations, out_status, (hipStream_t)stream);
}

size_t mpl_smooth_tracks_workspace_bytes(long long frames, int joints, int n_segments) {
    return smooth_tracks_workspace_bytes(frames, joints, n_segments);
}

int mpl_smooth_tracks(const float* points, const float* weight, const int* segments, const int* seg_offsets_dev, int n_segments,
                      long long frames, int joints, double smoothness, int order, double huber, int max_iterations,
                      double step_tolerance, unsigned flags, void* workspace, size_t workspace_bytes, float* out_points,
                      float* out_residual, float* out_irls, double* out_cost0, double* out_cost, int* out_iterations,
                      unsigned char* out_status, double* out_points64, void* stream) {
    clear_stale_hip_error();
    return launch_smooth_tracks(points, weight, segments, seg_offsets_dev, n_segments, frames, joints, smoothness, order, huber,
                                max_iterations, step_tolerance, flags, workspace, workspace_bytes, out_points, out_residual, out_irls,
                                out_cost0, out_cost, out_iterations, out_status, out_points64, (hipStream_t)stream);
}

size_t mpl_locate_cameras_workspace_bytes(int batch, int views, int joints) { return locate_cameras_workspace_bytes(batch, views, joints); }

int mpl_locate_cameras(const float* points, const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev,
                       int batch, int views, int joints, double threshold, int hypotheses, const unsigned long long* keys,
                       unsigned fixed_mask, void* workspace, size_t workspace_bytes, double* out_cams, float* out_inliers, int* out_count,
                       int* out_best, double* out_error, unsigned char* out_status, double* out_poses, double* out_scores, void* stream) {
    clear_stale_hip_error();
    return launch_locate_cameras(points, pixels, conf, cams_dev, dist_dev, batch, views, joints, threshold, hypotheses, keys, fixed_mask,
                                 workspace, workspace_bytes, out_cams, out_inliers, out_count, out_best, out_error, out_status, out_poses,
                                 out_scores, (hipStream_t)stream);
}

size_t mpl_relative_pose_workspace_bytes(int batch, int pairs, int joints) { return relative_pose_workspace_bytes(batch, pairs, joints); }

int mpl_relative_pose(const float* pixels, const float* conf, const double* cams_dev, const double* dist_dev, int batch, int views,
                      int joints, const int* pairs, int n_pairs, double threshold, int hypotheses, const unsigned long long* keys,
                      double baseline, void* workspace, size_t workspace_bytes, double* out_rotation, double* out_direction,
                      double* out_cams, float* out_inliers, int* out_count, int* out_best, double* out_error, unsigned char* out_status,
                      double* out_poses, double* out_scores, int* out_roots, void* stream) {
    clear_stale_hip_error();
    return launch_relative_pose(pixels, conf, cams_dev, dist_dev, batch, views, joints, pairs, n_pairs, threshold, hypotheses, keys,
                                baseline, workspace, workspace_bytes, out_rotation, out_direction, out_cams, out_inliers, out_count,
                                out_best, out_error, out_status, out_poses, out_scores, out_roots, (hipStream_t)stream);
}

int mpl_refine_relative_pose(const float* pixels, const float* conf, const float* weight, const double* cams_dev, const double* dist_dev,
                             int batch, int views, int joints, const int* pairs, int n_pairs, const double* rotation,
                             const double* direction, double huber, int max_iterations, double step_tolerance, double baseline,
                             double* out_rotation, double* out_direction, double* out_cams, double* out_error, double* out_cost0,
                             double* out_cost, int* out_used, int* out_iterations, unsigned char* out_status, void* stream) {
    clear_stale_hip_error();
    return launch_refine_relative_pose(pixels, conf, weight, cams_dev, dist_dev, batch, views, joints, pairs, n_pairs, rotation, direction,
                                       huber, max_iterations, step_tolerance, baseline, out_rotation, out_direction, out_cams, out_error,
                                       out_cost0, out_cost, out_used, out_iterations, out_status, (hipStream_t)stream);
}

int mpl_procrustes_align(const float* pred, const float* target, const float* conf, const int* sel, int n_sel, const float* scale3,
                         const float* offset3, int scaling, int reflection, int batch, int joints, float* aligned, float* d,
                         float* rotation, float* scale, float* translation, void* stream) {
    clear_stale_hip_error();
    return launch_procrustes_align(pred, target, conf, sel, n_sel, scale3, offset3, scaling, reflection, batch, joints, aligned, d,
                                   rotation, scale, translation, (hipStream_t)stream);
}

int mpl_pose_metrics_size(int joints) { return 4 + 2 * (joints + 1) + 3 * joints + 3; }

int mpl_pose_metrics(const float* output, const float* target, const float* weight, int batch, int joints,
                     const float* scale3, const float* offset3, float* result, void* stream) {
    clear_stale_hip_error();
    if (int rc = earlier_device_failure()) return rc;
    return launch_pose_metrics(output, target, weight, batch, joints, scale3, offset3, 0u, result, (hipStream_t)stream);
}

int mpl_pose_metrics_ex(const float* output, const float* target, const float* weight, int batch, int joints,
                        const float* scale3, const float* offset3, uint32_t not_consider_mask, float* result, void* stream) {
    clear_stale_hip_error();
    if (int rc = earlier_device_failure()) return rc;
    return launch_pose_metrics(output, target, weight, batch, joints, scale3, offset3, not_consider_mask, result, (hipStream_t)stream);
}

size_t mpl_eval_state_bytes(int n_sel, int n_groups) { return eval_state_bytes(n_sel, n_groups); }

int mpl_eval_reset(void* state, int n_sel, int n_groups, void* stream) {
    clear_stale_hip_error();
    return launch_eval_reset(state, n_sel, n_groups, (hipStream_t)stream);
}

int mpl_eval_accumulate(void* state, const mpl_eval_options* opt, const float* output, const float* x1, const float* x2,
                        const float* target, const float* weight, const float* conf_3d, const int32_t* group, int batch, int joints,
                        float* keep_pred, float* keep_tgt, long long keep_capacity, void* stream) {
    clear_stale_hip_error();
    if (int rc = earlier_device_failure()) return rc;
    return launch_eval_accumulate(state, opt, output, x1, x2, target, weight, conf_3d, group, batch, joints, keep_pred, keep_tgt,
                                  keep_capacity, (hipStream_t)stream);
}

int mpl_eval_report_size(int n_sel, int n_groups) { return eval_report_doubles(n_sel, n_groups); }

int mpl_eval_report(const void* state, int n_sel, int n_groups, uint64_t not_consider_mask, double* report, void* stream) {
    clear_stale_hip_error();
    return launch_eval_report(state, n_sel, n_groups, not_consider_mask, report, (hipStream_t)stream);
}

int mpl_forward(const mpl_config* cfg, const mpl_weights* w, const mpl_inputs* in, float* out, void* workspace,
                size_t workspace_bytes, void* stream) {
    clear_stale_hip_error();
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if ((rc = mpl_config_supported(cfg))) return rc;
    if ((rc = earlier_device_failure())) return rc;
    if (!w || !in || !out || in->batch <= 0) return MPL_E_INVALID;
    if ((long long)in->batch * cfg->num_views * cfg->num_joints > (1ll << 30)) return MPL_E_UNSUPPORTED;
    if (!(cfg->flags & MPL_F_NO_FPT) && cfg->depth > 0) {      // the block stack's GEMMs must take its rows (block_stack_impl)
        const bool kp = (cfg->flags & MPL_F_KPTOK) != 0;
        const int Ds = kp ? cfg->dim : mpl_fpt_width(cfg);
        if (!ln_gemm_rows_ok((long long)in->batch * cfg->num_views * (kp ? cfg->num_joints : 1), Ds, Ds)) return MPL_E_UNSUPPORTED;
    }
    const size_t need = mpl_forward_workspace_bytes(cfg, in->batch);
    if (!workspace || workspace_bytes < need) return MPL_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int B = in->batch, V = cfg->num_views, D = mpl_fpt_width(cfg);
    float* xs = reinterpret_cast<float*>(workspace);
    char* rest = reinterpret_cast<char*>(workspace) + align_up((size_t)B * V * D * sizeof(float), 256);
    const size_t rest_bytes = workspace_bytes - (size_t)(rest - reinterpret_cast<char*>(workspace));

    if ((rc = launch_spt(cfg, w, in, xs, w->spt_packed != 0, s))) return rc;

    const unsigned* err_ws = nullptr;     // set by the block stack when it runs as the persistent launch
    if (!(cfg->flags & MPL_F_NO_FPT) && cfg->depth > 0) {
        // forward_features :420-423: the last block is applied twice
        uint8_t sched[MPL_MAX_APPS];
        int n = 0;
        for (int l = 0; l < cfg->depth; ++l) {
            if (n + 2 > MPL_MAX_APPS) return MPL_E_UNSUPPORTED;
            if (l == cfg->depth - 1) sched[n++] = (uint8_t)l;
            sched[n++] = (uint8_t)l;
        }
        const bool kp = (cfg->flags & MPL_F_KPTOK) != 0;
        if ((rc = block_stack_impl(xs, B, kp ? V * cfg->num_joints : V, kp ? cfg->dim : D, cfg->heads, w->fpt_blocks,
                                   sched, n, rest, rest_bytes, &err_ws, (cfg->flags & MPL_F_NO_SMALL_STACK) == 0, s)))
            return rc;
    }
    return launch_fuse_head(cfg, w, xs, B, out, nullptr, err_ws, s);
}

}  // extern "C"
