// compact_kernels.hip -- the scan between the verdict and the commit kernel of a call that
// compacts its flagged rows (wgcs_compact.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgcs_compact.h"

namespace wgcs {

namespace {

// One block: block_count[b] becomes the flagged rows of the blocks below b, 1,024 blocks a turn,
// and *count the entries the commit kernel writes.
__global__ __launch_bounds__(kScanThreads) void compact_scan_kernel(uint32_t* __restrict__ block_count,
                                                                    uint32_t n_blocks, uint32_t cap,
                                                                    uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_sum[kScanThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  uint32_t below = 0;  // the flagged rows of every block of the turns before this one
  for (uint32_t first = 0; first < n_blocks; first += kScanThreads) {
    const uint32_t b = first + threadIdx.x;
    const uint32_t mine = b < n_blocks ? block_count[b] : 0;
    const uint32_t x = wave_scan(mine, lane, WaveSum());
    if (lane == kWave - 1) wave_sum[wave] = x;
    __syncthreads();
    uint32_t waves_below = 0, turn = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScanThreads / kWave; ++w) {
      const uint32_t s = wave_sum[w];
      if (w < wave) waves_below += s;
      turn += s;
    }
    if (b < n_blocks) block_count[b] = below + waves_below + x - mine;
    below += turn;
    __syncthreads();  // wave_sum is written again in the next turn
  }
  if (threadIdx.x == 0) *count = below < cap ? below : cap;
}

}  // namespace

hipError_t launch_compact_scan(uint32_t* block_count, uint32_t n_blocks, uint32_t cap, uint32_t* count,
                               hipStream_t s) {
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_count, n_blocks, cap, count);
  return hipGetLastError();
}

}  // namespace wgcs
