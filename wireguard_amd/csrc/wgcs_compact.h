// wgcs_compact.h -- count, scan, rank: the rows of a call that pass a verdict, compacted in row
// order into a dense list of at most cap entries, the entries past the count filled as a tail.
// wgcs_handshake_accept_batch (winners into response descriptors), wgcs_rekey_start_batch
// (candidates into start descriptors) and wgcs_timers_expire_batch (owing rows into keepalive
// jobs) share it; their kernel files keep the row functions, the flag and the tail fill.
// wgcs_staged_release_batch (ready peers into send jobs, a peer taking as many entries as it has
// staged packets) uses the weighted form at the end of this file with the same scan kernel.
//
//   verdict kernel   one lane per row, kCompactThreads a block: judges its row, and
//                    compact_count_block stores the flagged rows of the block in block_count[b]
//   scan kernel      compact_kernels.hip, one block: block_count[b] becomes the flagged rows of
//                    the blocks below b, and *count = min(all flagged rows, cap)
//   commit kernel    a grid over max(rows, cap): lane q reads its row's flag again, takes its
//                    rank from compact_rank and commits entry rank if it is below cap, and fills
//                    entry q if cap > q >= *count
//
// The rank of a flagged row -- the flagged rows below it -- is a sum of whole-block counts and of
// a ballot inside its block, so it does not depend on the order the blocks or waves ran in.  A
// flagged row's entry lies below the count and a tail entry at or past it, so no two lanes write
// one entry.  block_count is scratch of compact_blocks(rows) words, which the call owns from the
// verdict launch until the commit is done.  No lane of a verdict or commit kernel may return
// before the block-wide helper: both hold a barrier.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgcs_kernels.h"
#include "wgcs_wave.h"

namespace wgcs {

constexpr int kCompactThreads = 256;
constexpr int kScanThreads = 1024;

inline uint32_t compact_blocks(uint32_t n) { return n / kCompactThreads + (n % kCompactThreads != 0); }

// The launches of one call on s: verdict(n_blocks) issues the caller's launches that end in
// compact_count_block over n_blocks blocks, commit(n_blocks) its commit launch; both return the
// launch's error.  Without rows there is no verdict launch, but always a scan, which writes
// *count; the commit grid covers the rows and the cap, and is skipped when both are 0.
template <typename Verdict, typename Commit>
hipError_t launch_compact(uint32_t n_rows, uint32_t cap, uint32_t* block_count, uint32_t* count, hipStream_t s,
                          Verdict verdict, Commit commit) {
  const uint32_t n_blocks = compact_blocks(n_rows);
  hipError_t e;
  if (n_blocks && (e = verdict(n_blocks)) != hipSuccess) return e;
  if ((e = launch_compact_scan(block_count, n_blocks, cap, count, s)) != hipSuccess) return e;
  const uint32_t rows = n_rows > cap ? n_rows : cap;
  return rows ? commit(compact_blocks(rows)) : hipSuccess;
}

#ifdef __HIPCC__

// The tail of a verdict kernel, every lane of the block: block_count[blockIdx.x] = its flagged rows.
__device__ inline void compact_count_block(bool flag, uint32_t* __restrict__ block_count) {
  const int flagged = __syncthreads_count(flag);
  if (threadIdx.x == 0) block_count[blockIdx.x] = (uint32_t)flagged;
}

// The rank of a flagged lane of a commit kernel (any value in the others), every lane of the
// block; below is block_count behind the scan.  Only a flagged lane reads below[blockIdx.x]: a
// commit block past the verdict kernel's grid, which fills tail entries only, has no word there.
__device__ inline uint32_t compact_rank(bool flag, const uint32_t* __restrict__ below) {
  __shared__ uint32_t wave_flagged[kCompactThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint64_t ballot = __ballot(flag);
  if (lane == 0) wave_flagged[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  uint32_t rank = 0;
  if (flag) {
    rank = below[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_flagged[w];
  }
  return rank;
}

// The weighted form (wgcs_staged_release_batch): a row takes w entries of the list, not one, so
// the block word is the sum of the weights and a row's rank the weight of the rows below it.  The
// scan is the same kernel -- it adds the block words whatever they count -- and *count comes out
// as min(all weight, cap); a caller whose list ends at the first row that does not fit corrects
// it in its commit kernel.  The sum of all weights stays below 2^32.

// The tail of a weighted verdict kernel, every lane of the block: block_weight[blockIdx.x] = the
// weights of its rows (0 for a row that is not flagged).
__device__ inline void compact_weigh_block(uint32_t w, uint32_t* __restrict__ block_weight) {
  __shared__ uint32_t wave_weight[kCompactThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint32_t x = wave_sum(w);
  if (lane == 0) wave_weight[wave] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t v = 0; v < kCompactThreads / kWave; ++v) sum += wave_weight[v];
    block_weight[blockIdx.x] = sum;
  }
}

// The weight of the rows below a lane of a weighted commit kernel, every lane of the block; below
// is block_weight behind the scan, read by the lanes with w != 0 only.
__device__ inline uint32_t compact_weighted_rank(uint32_t w, const uint32_t* __restrict__ below) {
  __shared__ uint32_t wave_weight[kCompactThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint32_t x = wave_scan(w, lane, WaveSum());  // the weights of the wave's lanes up to this one
  if (lane == kWave - 1) wave_weight[wave] = x;
  __syncthreads();
  uint32_t rank = 0;
  if (w) {
    rank = below[blockIdx.x] + x - w;
    for (uint32_t v = 0; v < wave; ++v) rank += wave_weight[v];
  }
  return rank;
}

#endif  // __HIPCC__

}  // namespace wgcs
