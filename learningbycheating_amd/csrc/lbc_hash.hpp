// Counter-based random numbers shared by the device-side input pipeline (data.hip: per-pixel augmentation noise) and the replay
// buffer's sampler (replay.hip): no generator state on the device, draw = hash of (seed, two counters).
#pragma once
#include <hip/hip_runtime.h>

static __device__ __forceinline__ unsigned hash_u32(unsigned x)
{
    // "lowbias32" integer finaliser (public domain, Chris Wellons): full avalanche in 2 multiplies
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
static __device__ __forceinline__ unsigned hash3(unsigned seed, unsigned a, unsigned b) { return hash_u32(seed ^ hash_u32(a * 0x9E3779B9U + hash_u32(b + 0x85EBCA6BU))); }
