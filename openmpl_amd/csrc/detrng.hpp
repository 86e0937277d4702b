// The counter-based random numbers of openmpl_amd/detrng.py on the device, stated once: synth.hip and heatmap_render.hip draw
// through this header only.  draw(key, i) = mix(key + (i + 1) * GOLD), top 53 bits -> [0,1); the keys come from the host
// (detrng._stream_key).
#pragma once
#include "common.hpp"

namespace mpl {

// SplitMix64's finaliser
__device__ __forceinline__ unsigned long long detrng_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// detrng.uniform01: element i of the stream `key`, a double in [0,1) with 53 bits
__device__ __forceinline__ double detrng_draw(unsigned long long key, unsigned long long i) {
    return (double)(detrng_mix(key + (i + 1ull) * 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace mpl
