// timers_kernels.hip -- the peer timers on device-resident tables
// (include/wgcsum.h).  The event calls are the bodies of wgcs_timers.h under
// the one kernel of wgcs_each.h, instantiated below:
//   TimersSent         behind send-assign                      send.go:498-510
//   TimersReceived     over the write groups                   receive.go:486-494
//   TimersFresh        !isRetry over the peer rows             send.go:85-87
//   TimersInitiated    over the start call's tickets           send.go:117-126
//   TimersResponded    behind respond                          receive.go:311-312, send.go:158-160
//   TimersFinished     behind begin-initiator                  receive.go:339-348
//   TimersRotated      behind keypairs-received                receive.go:422-427
// and the expiry keeps kernels of its own:
//   expire             the five expiry bodies over the peer rows   timers.go:73-144
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
#include "wgcs_each.h"
#include "wgcs_kernels.h"
#include "wgcs_timers.h"

namespace wgcs {

template hipError_t launch_each(const TimersSent&, uint32_t, hipStream_t);
template hipError_t launch_each(const TimersReceived&, uint32_t, hipStream_t);
template hipError_t launch_each(const TimersFresh&, uint32_t, hipStream_t);
template hipError_t launch_each(const TimersInitiated&, uint32_t, hipStream_t);
template hipError_t launch_each(const TimersResponded&, uint32_t, hipStream_t);
template hipError_t launch_each(const TimersFinished&, uint32_t, hipStream_t);
template hipError_t launch_each(const TimersRotated&, uint32_t, hipStream_t);

namespace {

constexpr int kThreads = kCompactThreads;

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
