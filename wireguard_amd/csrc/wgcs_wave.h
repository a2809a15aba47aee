// wgcs_wave.h -- the wave64 primitives of the per-key and the compacting kernels (wgcs_keyorder.h,
// wgcs_compact.h): a lane of a 64-bit value, the wave-scope fence, one inclusive scan and one sum.
// Device only.  Every lane of the wave calls them together.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wgcs {

constexpr int kWave = 64;  // gfx950 runs these kernels in wave64

#ifdef __HIPCC__

__device__ inline uint64_t readlane64(uint64_t x, int lane) {  // lane is wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// LDS traffic of one wave to memory that only this wave touches: program order is execution
// order on the hardware, so all that is needed is that the compiler keeps it
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// clang-format off
struct WaveSum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct WaveMax { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
// clang-format on

// op over x of the wave's lanes up to and including this one (uint32_t or uint64_t, WaveSum or
// WaveMax); lane is the lane's place in the wave.  Lane 63 holds op over the whole wave.
template <typename T, typename Op>
__device__ inline T wave_scan(T x, uint32_t lane, Op op) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const T y = __shfl_up(x, d, kWave);
    if (lane >= (uint32_t)d) x = op(x, y);
  }
  return x;
}

// the sum of x over the wave, in lane 0 (the other lanes hold partial sums)
__device__ inline uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_down(x, d, kWave);
  return x;
}

#endif  // __HIPCC__

}  // namespace wgcs
