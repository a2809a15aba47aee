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
//     timers_expire_verdict_kernel   every due timer of a row
//     timers_expire_commit_kernel    the keepalive job of every owing row that has room, and the tail jobs
//   The rows that owe a keepalive are compacted into the jobs by the scheme of wgcs_compact.h,
//   whose scan runs between the two.
// An event row costs two dependent loads (peer id -> peer row -> flags) and a
// few 32-bit atomics on one 64-byte row; rows of one peer only OR bits in, AND
// bits out or store what every row of the peer stores, so the table does not
// depend on which wave ran first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_compact.h"
#include "wgcs_kernels.h"
#include "wgcs_timers.h"

namespace wgcs {

namespace {

constexpr int kThreads = kCompactThreads;  // the one-lane-per-row kernels run the blocks of expire's two

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
  compact_count_block(owes, block_owe);
}

// The grid covers max(n_peers, n_ka_max) rows: lane q commits peer row q if it owes a job, and
// fills job q if it lies past the count.
__global__ __launch_bounds__(kThreads) void timers_expire_commit_kernel(
    wgcs_timers* timers, const wgcs_peer_key* __restrict__ table, uint32_t n_peers, uint32_t n_ka_max,
    uint32_t* __restrict__ ka_peer, int32_t* __restrict__ ka_count, int32_t* __restrict__ ka_sizes,
    int32_t* __restrict__ ka_status, const uint32_t* __restrict__ count, const uint32_t* __restrict__ owe_below,
    uint32_t* actions) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const bool owing = q < n_peers && (actions[q] & WGCS_TIMERS_ACT_KEEPALIVE) != 0;
  const uint32_t rank = compact_rank(owing, owe_below);
  if (owing) timers_expire_commit(q, rank, timers, table, n_ka_max, ka_peer, ka_count, ka_sizes, ka_status, actions);
  if (q < n_ka_max && q >= *count) timers_expire_tail(q, ka_peer, ka_count, ka_sizes, ka_status);
}

}  // namespace

hipError_t launch_timers_sent(const int32_t* sizes, const uint32_t* peer, const int32_t* count, const int32_t* status,
                              const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now, uint32_t seed,
                              const uint32_t* peer_rows, uint32_t n_ids, wgcs_timers* timers, uint32_t n_peers,
                              hipStream_t s) {
  hipLaunchKernelGGL(timers_sent_kernel, dim3(compact_blocks(n_jobs)), dim3(kThreads), 0, s, sizes, peer, count, status,
                     job_key, n_jobs, max_segs, now, seed, peer_rows, n_ids, timers, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_received(const wgcs_write_group* groups, uint32_t n, int64_t now, const uint32_t* peer_rows,
                                  uint32_t n_ids, wgcs_timers* timers, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_received_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, groups, n, now, peer_rows,
                     n_ids, timers, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_initiated(const uint32_t* reasons, const uint32_t* start_peer, const int32_t* init_status,
                                   uint32_t n_tickets, int64_t now, uint32_t seed, wgcs_timers* timers,
                                   uint32_t n_peers, hipStream_t s) {
  hipError_t e;
  if (n_peers) {
    hipLaunchKernelGGL(timers_fresh_kernel, dim3(compact_blocks(n_peers)), dim3(kThreads), 0, s, reasons, timers,
                       n_peers);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_tickets == 0 || n_peers == 0) return hipSuccess;
  hipLaunchKernelGGL(timers_initiated_kernel, dim3(compact_blocks(n_tickets)), dim3(kThreads), 0, s, start_peer,
                     init_status, n_tickets, now, seed, timers, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_responded(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now,
                                   wgcs_timers* timers, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_responded_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, resp, gate, n, now, timers,
                     n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_finished(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* gate,
                                  const int32_t* begun, uint32_t n, int64_t now, const wgcs_session_slot* hs_slots,
                                  uint32_t n_hs_slots, const wgcs_hs_state* states, uint32_t n_states,
                                  wgcs_timers* timers, wgcs_rekey* rekey, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_finished_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, arena, pkts, gate, begun, n,
                     now, hs_slots, n_hs_slots, states, n_states, timers, rekey, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_rotated(const wgcs_aead_pkt* pkts, const uint32_t* rotated, uint32_t n, int64_t now,
                                 const uint32_t* key_peer, uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids,
                                 wgcs_timers* timers, wgcs_rekey* rekey, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(timers_rotated_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, pkts, rotated, n, now,
                     key_peer, n_keys, peer_rows, n_ids, timers, rekey, n_peers);
  return hipGetLastError();
}

hipError_t launch_timers_expire(int64_t now, wgcs_timers* timers, wgcs_rekey* rekey, const wgcs_peer_key* table,
                                uint32_t n_peers, const uint32_t* staged, wgcs_keypairs* kp, wgcs_session_slot* slots,
                                uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                                wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys, uint32_t n_ka_max,
                                uint32_t* ka_peer, int32_t* ka_count, int32_t* ka_sizes, int32_t* ka_status,
                                uint32_t* n_ka, uint32_t* actions, uint32_t* block_owe, hipStream_t s) {
  return launch_compact(
      n_peers, n_ka_max, block_owe, n_ka, s,
      [&](uint32_t n_blocks) {
        hipLaunchKernelGGL(timers_expire_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, now, timers, rekey,
                           table, n_peers, staged, kp, slots, n_slots, peer_keys, n_peer_slots, keys, key_peer, n_keys,
                           actions, block_owe);
        return hipGetLastError();
      },
      [&](uint32_t n_blocks) {
        hipLaunchKernelGGL(timers_expire_commit_kernel, dim3(n_blocks), dim3(kThreads), 0, s, timers, table, n_peers,
                           n_ka_max, ka_peer, ka_count, ka_sizes, ka_status, n_ka, block_owe, actions);
        return hipGetLastError();
      });
}

}  // namespace wgcs
