// noise_accept_kernels.hip -- the responder's stateful tail on device-resident
// batches (include/wgcsum.h), device/noise.go:458-491 for a batch judged in row
// order under one clock value:
//   hs_accept_claim_kernel     the gate, the peer lookup, and the claim of every row its peer's
//                              stored state would accept                            :458-459
//   hs_accept_verdict_kernel   replay / flood against the claim's holder            :461-472
//   hs_accept_commit_kernel    the state update and the descriptor of every winner that has a
//                              ticket, and the tail descriptors                     :474-488
// The winners are compacted into the descriptors by the scheme of wgcs_compact.h, whose scan
// runs between verdict and commit.
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
// outcome does not depend on which wave ran first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_compact.h"
#include "wgcs_kernels.h"
#include "wgcs_noise.h"

namespace wgcs {

namespace {

constexpr int kThreads = kCompactThreads;  // claim runs the blocks of verdict and commit

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
  compact_count_block(q < n && v == WGCS_HS_ACCEPTED && gate[q] == WGCS_HS_CONSUMED, block_winners);
}

// The grid covers max(n, n_tickets) rows: lane q commits row q if it won, and fills descriptor
// q if it lies past the count.
__global__ __launch_bounds__(kThreads) void hs_accept_commit_kernel(
    const wgcs_hs_init* __restrict__ init, const int32_t* __restrict__ gate, uint32_t n, int64_t now,
    const uint32_t* __restrict__ peer_rows,
    wgcs_hs_peer* peers, const wgcs_hs_ticket* __restrict__ tickets, uint32_t n_tickets, wgcs_hs_resp* resp,
    const uint32_t* __restrict__ count, const uint32_t* __restrict__ winners_below, int32_t* __restrict__ verdict) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const bool won = q < n && verdict[q] == WGCS_HS_ACCEPTED && gate[q] == WGCS_HS_CONSUMED;
  const uint32_t rank = compact_rank(won, winners_below);
  if (won) verdict[q] = noise_accept_commit(q, rank, now, init, peer_rows, peers, tickets, n_tickets, resp);
  if (q < n_tickets && q >= *count) noise_accept_tail(resp + q);
}

}  // namespace

hipError_t launch_hs_accept(const wgcs_hs_init* init, const int32_t* gate, uint32_t n, int64_t now,
                            const wgcs_peer_key* table, const uint32_t* peer_rows, uint32_t n_ids, wgcs_hs_peer* peers,
                            uint32_t n_peers, const wgcs_hs_ticket* tickets, uint32_t n_tickets, wgcs_hs_resp* resp,
                            uint32_t* count, int32_t* verdict, uint32_t* block_winners, hipStream_t s) {
  return launch_compact(
      n, n_tickets, block_winners, count, s,
      [&](uint32_t n_blocks) {
        hipLaunchKernelGGL(hs_accept_claim_kernel, dim3(n_blocks), dim3(kThreads), 0, s, init, gate, n, now, table,
                           peer_rows, n_ids, peers, n_peers, verdict);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hs_accept_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, init, gate, n, peer_rows,
                           peers, verdict, block_winners);
        return hipGetLastError();
      },
      [&](uint32_t n_blocks) {
        hipLaunchKernelGGL(hs_accept_commit_kernel, dim3(n_blocks), dim3(kThreads), 0, s, init, gate, n, now,
                           peer_rows, peers, tickets, n_tickets, resp, count, block_winners, verdict);
        return hipGetLastError();
      });
}

}  // namespace wgcs
