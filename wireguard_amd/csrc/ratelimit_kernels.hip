// ratelimit_kernels.hip -- the rate limiter between the handshake screen and the
// Noise code on device-resident batches (include/wgcsum.h; ratelimiter/ratelimiter.go,
// device/receive.go:283-286), the row functions of wgcs_ratelimit.h one lane per row:
//   find       row q finds the slot of its source address or claims an empty one, and
//              writes the slot as its key (n_slots: the row is not charged)
//   position   behind the key order (wgcs_keyorder.h) over the slots: the first row of a
//              slot's run reads the entry, decides the run's first five rows and writes the
//              entry back; a row six or more into its run refuses itself
//   cleanup    old slot i moves into the new table unless it is idle
//
// Nothing here waits for another lane, and no loop's trip count depends on how many
// rows share an address: find's loop is the probe, at most n_slots steps plus one
// second look per slot (below); position looks at most five positions back and four
// ahead.  A run of 65,536 rows costs each of its lanes what a run of one costs.
//
// The table's first insert from the device.  Inside find the only table word that
// changes is `state`, 0 -> WGCS_RL_CLAIMED | row by atomicCAS, read by agent-scope
// atomic loads, so the private L2s of the eight XCDs and the L1s never serve a copy of
// it; everything else find reads (ip and family of live entries, d_src) was written
// before the launch.  A stale 0 costs a CAS that fails and returns the claim.  Between
// find and position lies the kernel boundary, and in position one lane owns an entry.
//
// A flood from one address brings thousands of lanes to one empty slot at once.  A lane
// whose lower neighbour in the wave stands at the same slot steps back from the CAS
// once and looks again: by then the neighbour's CAS has returned (the wave waited for
// it), the slot reads as claimed and the lane compares keys.  The second look is
// unconditional -- if the word still reads 0 the lane swaps for itself -- so this is
// one more trip round the loop, not a wait.  It brings the swaps on the hot word down
// from one per row to about one per wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_ratelimit.h"

namespace wgcs {

namespace {

constexpr int kThreads = kKeyOrderThreads;

// counts[] of every lane of the block into stats[]: a wave sum, an LDS add per wave, one
// global atomic per word and block.  Every lane of the block calls it.
__device__ inline void stats_add(const uint32_t counts[kRlStats], uint32_t* __restrict__ stats) {
  __shared__ uint32_t sum[kRlStats];
  if (threadIdx.x < kRlStats) sum[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRlStats; ++k) {
    const uint32_t v = wave_sum(counts[k]);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(&sum[k], v);
  }
  __syncthreads();
  if (threadIdx.x < kRlStats && sum[threadIdx.x]) atomicAdd(stats + threadIdx.x, sum[threadIdx.x]);
}

// verdict may alias gate: row q is read, then written, by the lane that owns it
__global__ __launch_bounds__(kThreads) void rl_find_kernel(const int32_t* gate, const wgcs_src_addr* __restrict__ src,
                                                           uint32_t n, wgcs_rl_entry* table, uint32_t n_slots,
                                                           int32_t* verdict, uint32_t* __restrict__ keys_in,
                                                           uint32_t* __restrict__ slots_in, uint32_t* stats) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  RlKey k = {0, {0, 0, 0, 0}};
  bool active = false, full = false, second = false;
  uint32_t s = 0, key = n_slots, left = n_slots;
  if (q < n) {
    const int32_t g = gate[q];
    if (g != WGCS_HS_PASS) verdict[q] = g;
    else if (!rl_key_of(src + q, &k)) verdict[q] = WGCS_ERR_INVALID_ARG;
    else {
      active = true;
      s = rl_home(k, n_slots);
    }
  }
  while (__any(active)) {  // the wave stays together: the neighbour's slot comes by a shuffle
    const uint32_t ps = __shfl_up(s, 1);
    const int pa = __shfl_up((int)active, 1);
    if (active) {
      const bool cas = second || lane == 0 || !pa || ps != s;
      const int r = rl_probe_step(table, s, q, k, src, n, cas);
      if (r > 0) {
        key = s;
        active = false;
      } else if (r < 0) {
        second = true;  // the same slot once more, then with the swap
      } else {
        second = false;
        s = (s + 1) & (n_slots - 1);
        if (--left == 0) {
          active = false;
          full = true;
          verdict[q] = WGCS_ERR_RATE_TABLE_FULL;
        }
      }
    }
  }
  if (q < n) keyorder_put(keys_in, slots_in, q, key);
  if (stats) {
    const uint32_t counts[kRlStats] = {0, 0, full ? 1u : 0u, 0};
    stats_add(counts, stats);
  }
}

__global__ __launch_bounds__(kThreads) void rl_position_kernel(const uint32_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ slots, uint32_t n,
                                                               uint32_t n_slots, const wgcs_src_addr* __restrict__ src,
                                                               wgcs_rl_entry* __restrict__ table, int64_t now,
                                                               int32_t* __restrict__ verdict, uint32_t* stats) {
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  uint32_t counts[kRlStats] = {0, 0, 0, 0};
  if (p < n) rl_position(p, keys, slots, n, n_slots, src, table, now, verdict, counts);
  if (stats) stats_add(counts, stats);
}

__global__ __launch_bounds__(kThreads) void rl_cleanup_kernel(const wgcs_rl_entry* __restrict__ old_table,
                                                              wgcs_rl_entry* new_table, uint32_t n_slots, int64_t now,
                                                              uint32_t* __restrict__ live) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const bool kept = i < n_slots && rl_cleanup_row(i, old_table, new_table, n_slots, now);
  const int count = __syncthreads_count(kept);
  if (threadIdx.x == 0 && count) atomicAdd(live, (uint32_t)count);
}

}  // namespace

hipError_t launch_ratelimit(const KeyOrder& ko, const int32_t* gate, const wgcs_src_addr* src, uint32_t n,
                            wgcs_rl_entry* table, uint32_t n_slots, int64_t now, int32_t* verdict, uint32_t* stats,
                            hipStream_t s) {
  hipError_t e;
  if (stats && (e = hipMemsetAsync(stats, 0, kRlStats * sizeof(uint32_t), s)) != hipSuccess) return e;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rl_find_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, gate, src, n, table, n_slots, verdict,
                     ko.keys_in, ko.slots_in, stats);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = keyorder_sort(ko, n, n_slots, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(rl_position_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, ko.keys, ko.slots, n, n_slots, src,
                     table, now, verdict, stats);
  return hipGetLastError();
}

hipError_t launch_ratelimit_cleanup(const wgcs_rl_entry* old_table, wgcs_rl_entry* new_table, uint32_t n_slots,
                                    int64_t now, uint32_t* live, hipStream_t s) {
  hipError_t e = hipMemsetAsync(new_table, 0, (size_t)n_slots * sizeof(wgcs_rl_entry), s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(live, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(rl_cleanup_kernel, dim3(keyorder_blocks(n_slots)), dim3(kThreads), 0, s, old_table, new_table, n_slots,
                     now, live);
  return hipGetLastError();
}

}  // namespace wgcs
