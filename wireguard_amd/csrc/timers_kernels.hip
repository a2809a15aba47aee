// timers_kernels.hip -- the peer timers on device-resident tables
// (include/wgcsum.h), the row functions of wgcs_timers.h one lane at a time:
//   timers_sent_kernel         behind send-assign                      send.go:498-510
//   timers_received_kernel     over the write groups                   receive.go:486-494
//   timers_fresh_kernel        !isRetry over the peer rows             send.go:85-87
//   timers_initiated_kernel    over the start call's tickets           send.go:117-126
//   timers_responded_kernel    behind respond                          receive.go:311-312, send.go:158-160
//   timers_finished_kernel     behind begin-initiator                  receive.go:339-348
//   timers_rotated_kernel      behind keypairs-received                receive.go:422-427
//   expire                     the five expiry bodies over the peer rows   timers.go:73-144
//     timers_expire_verdict_kernel   every due timer of a row, the rows of each block that owe a keepalive counted
//     timers_expire_scan_kernel      the block counts into the owing rows in front of each block, and *d_n_ka
//     timers_expire_commit_kernel    the keepalive job of every owing row that has room, and the tail jobs
// An event row costs two dependent loads (peer id -> peer row -> flags) and a
// few 32-bit atomics on one 64-byte row; rows of one peer only OR bits in, AND
// bits out or store what every row of the peer stores, so the table does not
// depend on which wave ran first.  The rank of an owing row is, as in the start
// call of rekey_kernels.hip, a sum of whole-block counts and of a ballot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_timers.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;  // gfx950 runs these kernels in wave64
constexpr int kScanThreads = 1024;

inline uint32_t blocks_for(uint32_t n) { return n / kThreads + (n % kThreads != 0); }

__global__ __launch_bounds__(kThreads) void timers_sent_kernel(
    const int32_t* __restrict__ sizes, const uint32_t* __restrict__ peer, const int32_t* __restrict__ count,
    const int32_t* __restrict__ status, const uint32_t* __restrict__ job_key, uint32_t n_jobs, uint32_t max_segs,
    int64_t now, uint32_t seed, const uint32_t* __restrict__ peer_rows, uint32_t n_ids, wgcs_timers* timers,
    uint32_t n_peers) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_jobs) return;
  timers_sent(j, sizes, peer, count, status, job_key, max_segs, now, seed, peer_rows, n_ids, timers, n_peers);
}

__global__ __launch_bounds__(kThreads) void timers_received_kernel(const wgcs_write_group* __restrict__ groups,
                                                                   uint32_t n, int64_t now,
                                                                   const uint32_t* __restrict__ peer_rows,
                                                                   uint32_t n_ids, wgcs_timers* timers,
                                                                   uint32_t n_peers) {
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  timers_received(c, groups, now, peer_rows, n_ids, timers, n_peers);
}

__global__ __launch_bounds__(kThreads) void timers_fresh_kernel(const uint32_t* __restrict__ reasons,
                                                                wgcs_timers* timers, uint32_t n_peers) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= n_peers) return;
  timers_initiated_fresh(r, reasons, timers);
}

__global__ __launch_bounds__(kThreads) void timers_initiated_kernel(const uint32_t* __restrict__ start_peer,
                                                                    const int32_t* __restrict__ init_status,
                                                                    uint32_t n_tickets, int64_t now, uint32_t seed,
                                                                    wgcs_timers* timers, uint32_t n_peers) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_tickets) return;
  timers_initiated(k, start_peer, init_status, now, seed, timers, n_peers);
}

__global__ __launch_bounds__(kThreads) void timers_responded_kernel(const wgcs_hs_resp* __restrict__ resp,
                                                                    const int32_t* __restrict__ gate, uint32_t n,
                                                                    int64_t now, wgcs_timers* timers,
                                                                    uint32_t n_peers) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  timers_responded(j, resp, gate, now, timers, n_peers);
}

__global__ __launch_bounds__(kThreads) void timers_finished_kernel(
    const uint8_t* __restrict__ arena, const wgcs_aead_pkt* __restrict__ pkts, const int32_t* __restrict__ gate,
    const int32_t* __restrict__ begun, uint32_t n, int64_t now, const wgcs_session_slot* __restrict__ hs_slots,
    uint32_t n_hs_slots, const wgcs_hs_state* __restrict__ states, uint32_t n_states, wgcs_timers* timers,
    wgcs_rekey* rekey, uint32_t n_peers) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  timers_finished(q, arena, pkts, gate, begun, now, hs_slots, n_hs_slots, states, n_states, timers, rekey, n_peers);
}

__global__ __launch_bounds__(kThreads) void timers_rotated_kernel(
    const wgcs_aead_pkt* __restrict__ pkts, const uint32_t* __restrict__ rotated, uint32_t n, int64_t now,
    const uint32_t* __restrict__ key_peer, uint32_t n_keys, const uint32_t* __restrict__ peer_rows, uint32_t n_ids,
    wgcs_timers* timers, wgcs_rekey* rekey, uint32_t n_peers) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  timers_rotated(i, pkts, rotated, now, key_peer, n_keys, peer_rows, n_ids, timers, rekey, n_peers);
}

// block_owe[b] = the rows of block b that owe a keepalive job
__global__ __launch_bounds__(kThreads) void timers_expire_verdict_kernel(
    int64_t now, wgcs_timers* timers, wgcs_rekey* rekey, const wgcs_peer_key* __restrict__ table, uint32_t n_peers,
    const uint32_t* __restrict__ staged, wgcs_keypairs* kp, wgcs_session_slot* slots, uint32_t n_slots,
    wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys,
    uint32_t* __restrict__ actions, uint32_t* __restrict__ block_owe) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  const bool owes = r < n_peers && timers_expire_verdict(r, now, timers, rekey, table, staged, kp, slots, n_slots,
                                                         peer_keys, n_peer_slots, keys, key_peer, n_keys, actions);
  const int owing = __syncthreads_count(owes);
  if (threadIdx.x == 0) block_owe[blockIdx.x] = (uint32_t)owing;
}

// One block: block_owe[b] becomes the owing rows of the blocks below b, 1,024 blocks a turn, and
// *count the jobs the commit kernel writes.  The scan of rekey_start_scan_kernel.
__global__ __launch_bounds__(kScanThreads) void timers_expire_scan_kernel(uint32_t* __restrict__ block_owe,
                                                                          uint32_t n_blocks, uint32_t n_ka_max,
                                                                          uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_sum[kScanThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  uint32_t below = 0;  // the owing rows of every block of the turns before this one
  for (uint32_t first = 0; first < n_blocks; first += kScanThreads) {
    const uint32_t b = first + threadIdx.x;
    const uint32_t mine = b < n_blocks ? block_owe[b] : 0;
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
    if (b < n_blocks) block_owe[b] = below + waves_below + x - mine;
    below += turn;
    __syncthreads();  // wave_sum is written again in the next turn
  }
  if (threadIdx.x == 0) *count = below < n_ka_max ? below : n_ka_max;
}

// The grid covers max(n_peers, n_ka_max) rows: lane q commits peer row q if it owes a job, and
// fills job q if it lies past the count.  An owing row's job lies below the count, so no two
// lanes write one job.
__global__ __launch_bounds__(kThreads) void timers_expire_commit_kernel(
    wgcs_timers* timers, const wgcs_peer_key* __restrict__ table, uint32_t n_peers, uint32_t n_ka_max,
    uint32_t* __restrict__ ka_peer, int32_t* __restrict__ ka_count, int32_t* __restrict__ ka_sizes,
    int32_t* __restrict__ ka_status, const uint32_t* __restrict__ count, const uint32_t* __restrict__ owe_below,
    uint32_t* actions) {
  __shared__ uint32_t wave_owe[kThreads / kWave];
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const bool owing = q < n_peers && (actions[q] & WGCS_TIMERS_ACT_KEEPALIVE) != 0;
  const uint64_t ballot = __ballot(owing);
  if (lane == 0) wave_owe[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (owing) {  // a block with an owing row is a block of the verdict kernel's grid: owe_below has its word
    uint32_t rank = owe_below[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_owe[w];
    timers_expire_commit(q, rank, timers, table, n_ka_max, ka_peer, ka_count, ka_sizes, ka_status, actions);
  }
  if (q < n_ka_max && q >= *count) timers_expire_tail(q, ka_peer, ka_count, ka_sizes, ka_status);
}

}  // namespace

hipError_t launch_timers_sent(const int32_t* sizes, const uint32_t* peer, const int32_t* count, const int32_t* status,
                              const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now, uint32_t seed,
                              const uint32_t* peer_rows, uint32_t n_ids, wgcs_timers* timers, uint32_t n_peers,
                              hipStream_t s) {
  hipLaunchKernelGGL(timers_sent_kernel, dim3(blocks_for(n_jobs)), dim3(kThreads), 0, s, sizes, peer, count, status,
                     job_key, n_jobs, max_segs, now, seed, peer_rows, n_ids, timers, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_received(const wgcs_write_group* groups, uint32_t n, int64_t now, const uint32_t* peer_rows,
                                  uint32_t n_ids, wgcs_timers* timers, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_received_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, groups, n, now, peer_rows,
                     n_ids, timers, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_initiated(const uint32_t* reasons, const uint32_t* start_peer, const int32_t* init_status,
                                   uint32_t n_tickets, int64_t now, uint32_t seed, wgcs_timers* timers,
                                   uint32_t n_peers, hipStream_t s) {
  hipError_t e;
  if (n_peers) {
    hipLaunchKernelGGL(timers_fresh_kernel, dim3(blocks_for(n_peers)), dim3(kThreads), 0, s, reasons, timers, n_peers);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_tickets == 0 || n_peers == 0) return hipSuccess;
  hipLaunchKernelGGL(timers_initiated_kernel, dim3(blocks_for(n_tickets)), dim3(kThreads), 0, s, start_peer,
                     init_status, n_tickets, now, seed, timers, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_responded(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now,
                                   wgcs_timers* timers, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_responded_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, resp, gate, n, now, timers,
                     n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_finished(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* gate,
                                  const int32_t* begun, uint32_t n, int64_t now, const wgcs_session_slot* hs_slots,
                                  uint32_t n_hs_slots, const wgcs_hs_state* states, uint32_t n_states,
                                  wgcs_timers* timers, wgcs_rekey* rekey, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_finished_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, arena, pkts, gate, begun, n,
                     now, hs_slots, n_hs_slots, states, n_states, timers, rekey, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_rotated(const wgcs_aead_pkt* pkts, const uint32_t* rotated, uint32_t n, int64_t now,
                                 const uint32_t* key_peer, uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids,
                                 wgcs_timers* timers, wgcs_rekey* rekey, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_rotated_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, pkts, rotated, n, now, key_peer,
                     n_keys, peer_rows, n_ids, timers, rekey, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_expire(int64_t now, wgcs_timers* timers, wgcs_rekey* rekey, const wgcs_peer_key* table,
                                uint32_t n_peers, const uint32_t* staged, wgcs_keypairs* kp, wgcs_session_slot* slots,
                                uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                                wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys, uint32_t n_ka_max,
                                uint32_t* ka_peer, int32_t* ka_count, int32_t* ka_sizes, int32_t* ka_status,
                                uint32_t* n_ka, uint32_t* actions, uint32_t* block_owe, hipStream_t s) {
  const uint32_t n_blocks = blocks_for(n_peers);
  hipError_t e;
  if (n_blocks) {
    hipLaunchKernelGGL(timers_expire_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, now, timers, rekey, table,
                       n_peers, staged, kp, slots, n_slots, peer_keys, n_peer_slots, keys, key_peer, n_keys, actions,
                       block_owe);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(timers_expire_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_owe, n_blocks, n_ka_max, n_ka);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t rows = n_peers > n_ka_max ? n_peers : n_ka_max;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(timers_expire_commit_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, s, timers, table, n_peers,
                     n_ka_max, ka_peer, ka_count, ka_sizes, ka_status, n_ka, block_owe, actions);
  return hipGetLastError();
}

}  // namespace wgcs
