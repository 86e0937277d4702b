// Hypothesise-and-score, the scaffold of locate_cameras.hip and relative_pose.hip, each piece once.  A call
// works on units (views there, pairs here) of N slots each, in three launches: a prepare kernel, one workgroup of THREADS per unit;
// a hypothesis kernel, one lane per hypothesis and one wave per workgroup, which draws a sample, solves and scores; a select
// kernel, one workgroup of THREADS per unit.  Here: the sum of a workgroup, the draw of distinct participating slots, the place and
// the void form of a hypothesis, the tiled scoring loop, the total order of hypotheses with its reduction and the `located` rule,
// the host refusals both calls share and their three profiled launches.  A file keeps what is its own: the workspace layout, the
// participation rule, the solver, the residual and the outputs of its select kernel.  Device and launch side only.
#pragma once
#include "common.hpp"
#include "detrng.hpp"

namespace mpl {
namespace consensus {

constexpr int LANES = 64;                // hypotheses of one workgroup of a hypothesis kernel: one wave
constexpr int TILE = 64;                 // slots staged in LDS at a time: one per lane
constexpr int ATTEMPTS = 16;             // draws for one slot of a sample
constexpr int THREADS = 256, WAVES = THREADS / 64;       // of a prepare or select workgroup
constexpr int MIN_INLIERS = 6;           // a winner with fewer locates nothing
constexpr int MAX_HYPOTHESES = 65536;

// the sums of a workgroup of THREADS: down each wave by shuffles, then across the waves in their order; every thread gets them
template <int K, int KP>
__device__ __forceinline__ void block_sum(double (&a)[K], double (*sh_part)[KP], double* sh_tot) {
    static_assert(K <= KP, "sh_part holds K sums a wave");
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += __shfl_down(a[k], off, 64);
    }
    __syncthreads();                                     // the last read of sh_tot is over
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh_part[wave][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double r = sh_part[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) r += sh_part[w][threadIdx.x];
        sh_tot[threadIdx.x] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = sh_tot[k];
}

// SAMPLE distinct participating slots of hypothesis h: slot k is the first of TRIES draws, counter ((h SAMPLE + k) TRIES + a), that
// takes part and is none of the slots before it -> false where one of them was not found (its pick is then 0).  Every draw is
// below N, so a lane beyond H draws like any other
template <int SAMPLE, int TRIES = ATTEMPTS, class TakesPart>
__device__ __forceinline__ bool draw_distinct(unsigned long long key, unsigned h, unsigned N, TakesPart takes_part_of_slot,
                                              unsigned (&pick)[SAMPLE]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < SAMPLE; ++k) {
        bool got = false;
        unsigned nk = 0;
        for (int a = 0; a < TRIES; ++a) {
            const unsigned n = (unsigned)(detrng_draw(key, ((unsigned long long)h * SAMPLE + k) * TRIES + a) * (double)N);
            bool good = !got && takes_part_of_slot(n);
#pragma unroll
            for (int i = 0; i < k; ++i) good = good && n != pick[i];
            if (good) {
                got = true;
                nk = n;
            }
        }
        pick[k] = nk;
        ok = ok && got;
    }
    return ok;
}

// Where hypothesis h of a unit is written: its pose (12) and its score (count, cost).  A lane beyond H goes along with its wave
// and writes nothing.  Void: a pose that is not a number, and the score (0, inf), which the select kernel passes over
struct Hypothesis {
    double* pose;
    double* score;
    bool live;
    __device__ __forceinline__ void write_score(bool valid, int count, double cost) const {
        if (!live) return;
        score[0] = valid ? (double)count : 0.0;
        score[1] = valid ? cost : __builtin_inf();
    }
    __device__ __forceinline__ void write_void() const {
        if (!live) return;
        for (int k = 0; k < 12; ++k) pose[k] = __builtin_nan("");
        write_score(false, 0, 0.0);
    }
};

__device__ __forceinline__ Hypothesis hypothesis_at(double* poses, double* scores, unsigned unit, unsigned H, unsigned h) {
    return Hypothesis{poses + ((size_t)unit * H + h) * 12, scores + ((size_t)unit * H + h) * 2, h < H};
}

// The score of one pose over all N slots of a unit, by a wave of LANES hypotheses: the records (REC values of T, the weight last;
// weight 0 = takes no part) are staged TILE at a time in `tile`, copied in units of COPY, and every lane reads the same address,
// a broadcast.  residual(r, counts) gives the squared distance of record r and whether the slot can be an inlier at all.  count =
// the inliers, cost = sum w min(r2, tau2); a lane sums in the order of the slots, so its bits do not depend on how the
// hypotheses are dealt to workgroups.  Every lane of the workgroup has to call (barriers).  The result goes by value: handed out
// through references, the compiler no longer vectorised the residual of relative_pose.hip as it had, and one of its sums was
// contracted the other way round -- other bits in the cost
struct Score {
    int count;
    double cost;
};

template <class T, int REC, class COPY, class Residual>
__device__ __forceinline__ Score score_tiled(const T* rec, unsigned N, T* tile, double tau2, Residual residual) {
    constexpr int COPIES = REC * sizeof(T) / sizeof(COPY);
    static_assert(COPIES * sizeof(COPY) == REC * sizeof(T), "a record is a whole number of copies");
    const unsigned lane = threadIdx.x;
    double cost = 0.0;
    int count = 0;
    for (unsigned base = 0; base < N; base += TILE) {
        __syncthreads();                                 // the tile before is read
        if (base + lane < N) {
            const COPY* g = reinterpret_cast<const COPY*>(rec + REC * (size_t)(base + lane));
            COPY* t = reinterpret_cast<COPY*>(tile + REC * lane);
#pragma unroll
            for (int k = 0; k < COPIES; ++k) t[k] = g[k];
        }
        __syncthreads();
        const unsigned n = min((unsigned)TILE, N - base);
        for (unsigned i = 0; i < n; ++i) {
            const T* r = tile + REC * i;                 // the same address in every lane
            const T w = r[REC - 1];
            if (!(w > (T)0)) continue;
            bool counts;
            const double r2 = residual(r, counts);
            const bool in = counts && r2 <= tau2;
            count += in ? 1 : 0;
            cost += (double)w * (in ? r2 : tau2);
        }
    }
    return Score{count, cost};
}

// The order of hypotheses: most inliers, then the lowest cost, then the lowest number, among the ones that are not void (h < 0:
// none).  A total order, so any reduction tree gives the same winner
struct Winner {
    double count, cost;
    int h;
    __device__ __forceinline__ bool located() const { return h >= 0 && count >= (double)MIN_INLIERS; }
};

__device__ __forceinline__ bool better(const Winner& o, const Winner& b) {
    return o.h >= 0 && (b.h < 0 || o.count > b.count || (o.count == b.count && (o.cost < b.cost || (o.cost == b.cost && o.h < b.h))));
}

// the winner among the H scores (count, cost) of a unit, for every thread of a workgroup of THREADS; searched = false: none.  The
// pointer to the unit's scores is formed under `searched`, not before: the compiler then still sees that the winner is the same in
// every lane, and what the select kernels compute from it stays in scalar registers
__device__ __forceinline__ Winner select_winner(const double* scores, unsigned unit, unsigned H, bool searched) {
    __shared__ double sh_cnt[WAVES], sh_cost[WAVES];
    __shared__ int sh_h[WAVES];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Winner b{-1.0, __builtin_inf(), -1};
    if (searched) {
        const double* sc = scores + (size_t)unit * H * 2;
        for (unsigned h = threadIdx.x; h < H; h += THREADS) {
            const Winner o{sc[2 * (size_t)h], sc[2 * (size_t)h + 1], (int)h};
            if (!(o.cost <= FINITE_MAX)) continue;
            if (better(o, b)) b = o;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const Winner o{__shfl_down(b.count, off, 64), __shfl_down(b.cost, off, 64), __shfl_down(b.h, off, 64)};
        if (better(o, b)) b = o;
    }
    if (lane == 0) {
        sh_cnt[wave] = b.count; sh_cost[wave] = b.cost; sh_h[wave] = b.h;
    }
    __syncthreads();
    b = Winner{sh_cnt[0], sh_cost[0], sh_h[0]};
    for (int w = 1; w < WAVES; ++w) {
        const Winner o{sh_cnt[w], sh_cost[w], sh_h[w]};
        if (better(o, b)) b = o;
    }
    return b;
}

// ---- the launch side
// B samples, `units` views or pairs, J joints: what the three kernels index in 32 bits
inline bool sizes_ok(int B, int units, int J) {
    return B > 0 && units > 0 && J > 0 && units <= MPL_MAX_VIEWS && J <= 64 && (long long)B * units * J <= (1ll << 30);
}

// a threshold in pixels whose square is finite, and 1 .. MAX_HYPOTHESES hypotheses
inline int options_check(double threshold, int hypotheses) {
    if (!(threshold > 0.0) || !(threshold <= FINITE_MAX) || !(threshold * threshold <= FINITE_MAX) || hypotheses < 1 ||
        hypotheses > MAX_HYPOTHESES)
        return MPL_E_UNSUPPORTED;
    return MPL_OK;
}

template <class KERNEL, class PARAMS>
inline void launch_profiled(KERNEL kernel, dim3 grid, int threads, int lds, const PARAMS& p, hipStream_t s) {
    ProfScope prof(MPL_K_FUSE_HEAD, s);
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, p);
}

// The three launches of a call, each bracketed for the profiler.  Every kernel is named twice, compiled with the lens and without
// (the same one twice where it is not compiled both ways); lds: the dynamic LDS of the hypothesis kernel, opted into first
template <auto PREPARE_LENS, auto PREPARE, auto HYPOTHESES_LENS, auto HYPOTHESES, auto SELECT_LENS, auto SELECT, class PARAMS>
int launch(bool lens, unsigned units, unsigned H, int lds, const PARAMS& p, hipStream_t s) {
    if (const int e = lens ? kernel_lds_once<HYPOTHESES_LENS>(lds, LANES) : kernel_lds_once<HYPOTHESES>(lds, LANES)) return e;
    const dim3 each(units), hyp((H + LANES - 1) / LANES, units);
    launch_profiled(lens ? PREPARE_LENS : PREPARE, each, THREADS, 0, p, s);
    launch_profiled(lens ? HYPOTHESES_LENS : HYPOTHESES, hyp, LANES, lds, p, s);
    launch_profiled(lens ? SELECT_LENS : SELECT, each, THREADS, 0, p, s);
    return hip_check_launch();
}

}  // namespace consensus
}  // namespace mpl
