// noise_accept_kernels.hip -- the responder's stateful tail on device-resident
// batches (include/wgcsum.h), device/noise.go:458-491 for a batch judged in row
// order under one clock value:
//   hs_accept_claim_kernel     the gate, the peer lookup, and the claim of every row its peer's
//                              stored state would accept                            :458-459
//   hs_accept_verdict_kernel   replay / flood against the claim's holder, and the winners of
//                              each block counted                                  :461-472
//   hs_accept_scan_kernel      the block counts into the winners in front of each block, and
//                              *d_count
//   hs_accept_commit_kernel    the state update and the descriptor of every winner that has a
//                              ticket, and the tail descriptors                     :474-488
// One lane per row, as the kernels of noise_init_kernels.hip: a lane runs the row
// functions of wgcs_noise.h, which wgcs_handshake_accept_host runs too.  A lane
// reads the first 20 bytes of its wgcs_hs_init row (peer, sender, timestamp) and
// never its hash, chaining key or ephemeral.  Nothing draws randomness or reads
// a clock.
//
// Several rows of a batch may belong to one peer.  The claim kernel only reads
// the peer rows, but for an atomicMin of the row number into the peer's claim;
// the verdict kernel reads the claims and writes no peer row; the commit kernel
// lets each claim's holder write its peer row and give the claim back.  So the
// outcome does not depend on which wave ran first, and the rank of a winner --
// the winners in the rows below it -- is a sum of whole-block counts and of a
// ballot inside its block, whatever the order the blocks ran in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_noise.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;  // gfx950 runs these kernels in wave64
constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kThreads) void hs_accept_claim_kernel(const wgcs_hs_init* __restrict__ init,
                                                                   const int32_t* __restrict__ gate, uint32_t n,
                                                                   int64_t now, const wgcs_peer_key* __restrict__ table,
                                                                   const uint32_t* __restrict__ peer_rows,
                                                                   uint32_t n_ids, wgcs_hs_peer* peers,
                                                                   uint32_t n_peers, int32_t* __restrict__ verdict) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  verdict[q] = noise_accept_claim(q, init, gate, now, table, peer_rows, n_ids, peers, n_peers);
}

// block_winners[b] = the WGCS_HS_ACCEPTED rows of block b
__global__ __launch_bounds__(kThreads) void hs_accept_verdict_kernel(const wgcs_hs_init* __restrict__ init,
                                                                     const int32_t* __restrict__ gate, uint32_t n,
                                                                     const uint32_t* __restrict__ peer_rows,
                                                                     const wgcs_hs_peer* __restrict__ peers,
                                                                     int32_t* __restrict__ verdict,
                                                                     uint32_t* __restrict__ block_winners) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  int v = WGCS_HS_NONE;
  if (q < n) verdict[q] = v = noise_accept_verdict(q, verdict[q], init, n, peer_rows, peers);
  // a verdict passed through from the gate is no winner, whatever its value
  const int winners = __syncthreads_count(q < n && v == WGCS_HS_ACCEPTED && gate[q] == WGCS_HS_CONSUMED);
  if (threadIdx.x == 0) block_winners[blockIdx.x] = (uint32_t)winners;
}

// One block: block_winners[b] becomes the winners of the blocks below b, 1,024 blocks a turn,
// and *count the descriptors the commit kernel writes.
__global__ __launch_bounds__(kScanThreads) void hs_accept_scan_kernel(uint32_t* __restrict__ block_winners,
                                                                      uint32_t n_blocks, uint32_t n_tickets,
                                                                      uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_sum[kScanThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  uint32_t below = 0;  // the winners of every block of the turns before this one
  for (uint32_t first = 0; first < n_blocks; first += kScanThreads) {
    const uint32_t b = first + threadIdx.x;
    const uint32_t mine = b < n_blocks ? block_winners[b] : 0;
    uint32_t x = mine;  // the inclusive sum over the wave's lanes up to this one
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, kWave);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == kWave - 1) wave_sum[wave] = x;
    __syncthreads();
    uint32_t waves_below = 0, turn = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScanThreads / kWave; ++w) {
      const uint32_t s = wave_sum[w];
      if (w < wave) waves_below += s;
      turn += s;
    }
    if (b < n_blocks) block_winners[b] = below + waves_below + x - mine;
    below += turn;
    __syncthreads();  // wave_sum is written again in the next turn
  }
  if (threadIdx.x == 0) *count = below < n_tickets ? below : n_tickets;
}

// The grid covers max(n, n_tickets) rows: lane q commits row q if it won, and fills descriptor
// q if it lies past the count.  A winner's descriptor lies below the count, so no two lanes
// write one descriptor.
__global__ __launch_bounds__(kThreads) void hs_accept_commit_kernel(
    const wgcs_hs_init* __restrict__ init, const int32_t* __restrict__ gate, uint32_t n, int64_t now,
    const uint32_t* __restrict__ peer_rows,
    wgcs_hs_peer* peers, const wgcs_hs_ticket* __restrict__ tickets, uint32_t n_tickets, wgcs_hs_resp* resp,
    const uint32_t* __restrict__ count, const uint32_t* __restrict__ winners_below, int32_t* __restrict__ verdict) {
  __shared__ uint32_t wave_winners[kThreads / kWave];
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const bool won = q < n && verdict[q] == WGCS_HS_ACCEPTED && gate[q] == WGCS_HS_CONSUMED;
  const uint64_t ballot = __ballot(won);
  if (lane == 0) wave_winners[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (won) {  // a block with a winner is a block of the verdict kernel's grid: winners_below has its word
    uint32_t rank = winners_below[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_winners[w];
    verdict[q] = noise_accept_commit(q, rank, now, init, peer_rows, peers, tickets, n_tickets, resp);
  }
  if (q < n_tickets && q >= *count) noise_accept_tail(resp + q);
}

}  // namespace

hipError_t launch_hs_accept(const wgcs_hs_init* init, const int32_t* gate, uint32_t n, int64_t now,
                            const wgcs_peer_key* table, const uint32_t* peer_rows, uint32_t n_ids, wgcs_hs_peer* peers,
                            uint32_t n_peers, const wgcs_hs_ticket* tickets, uint32_t n_tickets, wgcs_hs_resp* resp,
                            uint32_t* count, int32_t* verdict, uint32_t* block_winners, hipStream_t s) {
  const uint32_t n_blocks = hs_accept_blocks(n);
  hipError_t e;
  if (n_blocks) {
    hipLaunchKernelGGL(hs_accept_claim_kernel, dim3(n_blocks), dim3(kThreads), 0, s, init, gate, n, now, table,
                       peer_rows, n_ids, peers, n_peers, verdict);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(hs_accept_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, init, gate, n, peer_rows,
                       peers, verdict, block_winners);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(hs_accept_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_winners, n_blocks, n_tickets,
                     count);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t rows = n > n_tickets ? n : n_tickets;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(hs_accept_commit_kernel, dim3(hs_accept_blocks(rows)), dim3(kThreads), 0, s, init, gate, n, now,
                     peer_rows, peers, tickets, n_tickets, resp, count, block_winners, verdict);
  return hipGetLastError();
}

}  // namespace wgcs
