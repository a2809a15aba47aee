// rekey_kernels.hip -- keypair expiry, the rekey rules and the start of a
// handshake on device-resident tables (include/wgcsum.h).  The per-entry calls
// are the bodies of wgcs_rekey.h under the one kernel of wgcs_each.h,
// instantiated below:
//   RekeyRecvGate      a packet under a keypair past RejectAfterTime      receive.go:162-170
//   RekeySendGate      a job without a usable current keypair             send.go:368-374
//   RekeySent          keepKeyFreshSending behind send-assign             send.go:213-227, :419-420
//   RekeyReceived      keepKeyFreshReceiving over the write groups        receive.go:80-91
//   RekeyResponded     lastSentHandshake behind respond                   send.go:131-133
// and the start call keeps kernels of its own:
//   start                      SendHandshakeInitiation over the peer rows         send.go:84-100
//     rekey_start_verdict_kernel   the wish and the timeout of every row
//     rekey_start_commit_kernel    the descriptor of every candidate that has a ticket, and the tail rows
//   The candidates are compacted into the descriptors by the scheme of wgcs_compact.h, whose
//   scan runs between the two.
// The gates are on the per-packet path: a row costs three dependent loads
// (key or peer id -> peer row -> keypair) and, when its keypair is stale, one
// store.  Rows of one peer only OR bits into its wgcs_rekey row or store the
// call's clock there, so the tables do not depend on which wave ran first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_compact.h"
#include "wgcs_each.h"
#include "wgcs_kernels.h"
#include "wgcs_rekey.h"

namespace wgcs {

template hipError_t launch_each(const RekeyRecvGate&, uint32_t, hipStream_t);
template hipError_t launch_each(const RekeySendGate&, uint32_t, hipStream_t);
template hipError_t launch_each(const RekeySent&, uint32_t, hipStream_t);
template hipError_t launch_each(const RekeyReceived&, uint32_t, hipStream_t);
template hipError_t launch_each(const RekeyResponded&, uint32_t, hipStream_t);

namespace {

constexpr int kThreads = kCompactThreads;

// block_cand[b] = the candidates of block b
__global__ __launch_bounds__(kThreads) void rekey_start_verdict_kernel(int64_t now, wgcs_rekey* rekey, uint32_t n_peers,
                                                                       int32_t* __restrict__ status,
                                                                       uint32_t* __restrict__ reasons,
                                                                       uint32_t* __restrict__ block_cand) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  int v = WGCS_HS_NONE;
  if (r < n_peers) status[r] = v = rekey_start_verdict(r, now, rekey, reasons);
  compact_count_block(r < n_peers && v == WGCS_HS_STARTED, block_cand);
}

// The grid covers max(n_peers, n_tickets) rows: lane q commits peer row q if it is a candidate,
// and fills descriptor q if it lies past the count.
__global__ __launch_bounds__(kThreads) void rekey_start_commit_kernel(
    int64_t now, wgcs_rekey* rekey, const wgcs_hs_peer* __restrict__ hs_peers, uint32_t n_peers,
    const wgcs_hs_start* __restrict__ tickets, uint32_t n_tickets, wgcs_hs_start* __restrict__ start,
    uint32_t* __restrict__ start_peer, const uint32_t* __restrict__ count, const uint32_t* __restrict__ cand_below,
    int32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const bool cand = q < n_peers && status[q] == WGCS_HS_STARTED;
  const uint32_t rank = compact_rank(cand, cand_below);
  if (cand) status[q] = rekey_start_commit(q, rank, now, rekey, hs_peers, tickets, n_tickets, start, start_peer);
  if (q < n_tickets && q >= *count) rekey_start_tail(q, start, start_peer);
}

}  // namespace

hipError_t launch_rekey_start(int64_t now, wgcs_rekey* rekey, const wgcs_hs_peer* hs_peers, uint32_t n_peers,
                              const wgcs_hs_start* tickets, uint32_t n_tickets, wgcs_hs_start* start,
                              uint32_t* start_peer, uint32_t* count, int32_t* status, uint32_t* reasons,
                              uint32_t* block_cand, hipStream_t s) {
  return launch_compact(
      n_peers, n_tickets, block_cand, count, s,
      [&](uint32_t n_blocks) {
        hipLaunchKernelGGL(rekey_start_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, now, rekey, n_peers,
                           status, reasons, block_cand);
        return hipGetLastError();
      },
      [&](uint32_t n_blocks) {
        hipLaunchKernelGGL(rekey_start_commit_kernel, dim3(n_blocks), dim3(kThreads), 0, s, now, rekey, hs_peers,
                           n_peers, tickets, n_tickets, start, start_peer, count, block_cand, status);
        return hipGetLastError();
      });
}

}  // namespace wgcs
