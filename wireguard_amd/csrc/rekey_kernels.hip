// rekey_kernels.hip -- keypair expiry, the rekey rules and the start of a
// handshake on device-resident tables (include/wgcsum.h), the row functions of
// wgcs_rekey.h one lane at a time:
//   rekey_recv_gate_kernel     a packet under a keypair past RejectAfterTime      receive.go:162-170
//   rekey_send_gate_kernel     a job without a usable current keypair             send.go:368-374
//   rekey_sent_kernel          keepKeyFreshSending behind send-assign             send.go:213-227, :419-420
//   rekey_received_kernel      keepKeyFreshReceiving over the write groups        receive.go:80-91
//   rekey_responded_kernel     lastSentHandshake behind respond                   send.go:131-133
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
#include "wgcs_kernels.h"
#include "wgcs_rekey.h"

namespace wgcs {

namespace {

constexpr int kThreads = kCompactThreads;  // the one-lane-per-row kernels run the blocks of start's two

__global__ __launch_bounds__(kThreads) void rekey_recv_gate_kernel(wgcs_aead_pkt* pkts, uint32_t n, int64_t now,
                                                                   const uint32_t* __restrict__ key_peer,
                                                                   uint32_t n_keys,
                                                                   const uint32_t* __restrict__ peer_rows,
                                                                   uint32_t n_ids,
                                                                   const wgcs_keypairs* __restrict__ kp,
                                                                   uint32_t n_peers) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (rekey_recv_expired(i, pkts, now, key_peer, n_keys, peer_rows, n_ids, kp, n_peers))
    pkts[i].key = WGCS_SESSION_EXPIRED;
}

// status_out may be status_in: a lane reads its own word and then writes it
__global__ __launch_bounds__(kThreads) void rekey_send_gate_kernel(
    const uint32_t* __restrict__ peer, const int32_t* __restrict__ count, const int32_t* status_in, uint32_t n_jobs,
    uint32_t max_segs, int64_t now, const uint32_t* __restrict__ peer_rows, uint32_t n_ids,
    const wgcs_keypairs* __restrict__ kp, uint32_t n_peers, const uint64_t* __restrict__ send_nonce, uint32_t n_keys,
    uint64_t limit, wgcs_rekey* rekey, int32_t* status_out) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_jobs) return;
  status_out[j] = rekey_send_gate(j, peer, count, status_in, max_segs, now, peer_rows, n_ids, kp, n_peers, send_nonce,
                                  n_keys, limit, rekey);
}

__global__ __launch_bounds__(kThreads) void rekey_sent_kernel(
    const uint32_t* __restrict__ peer, const int32_t* __restrict__ count, const int32_t* __restrict__ status,
    const uint32_t* __restrict__ job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now,
    const uint32_t* __restrict__ peer_rows, uint32_t n_ids, const wgcs_keypairs* __restrict__ kp, uint32_t n_peers,
    const uint64_t* __restrict__ send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_jobs) return;
  rekey_sent(j, peer, count, status, job_key, max_segs, now, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, limit,
             rekey);
}

__global__ __launch_bounds__(kThreads) void rekey_received_kernel(const wgcs_write_group* __restrict__ groups,
                                                                  uint32_t n, int64_t now,
                                                                  const uint32_t* __restrict__ peer_rows,
                                                                  uint32_t n_ids,
                                                                  const wgcs_keypairs* __restrict__ kp,
                                                                  uint32_t n_peers, wgcs_rekey* rekey) {
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  rekey_received(c, groups, now, peer_rows, n_ids, kp, n_peers, rekey);
}

__global__ __launch_bounds__(kThreads) void rekey_responded_kernel(const wgcs_hs_resp* __restrict__ resp,
                                                                   const int32_t* __restrict__ gate, uint32_t n,
                                                                   int64_t now, wgcs_rekey* rekey, uint32_t n_peers) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  rekey_responded(j, resp, gate, now, rekey, n_peers);
}

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

hipError_t launch_rekey_recv_gate(wgcs_aead_pkt* pkts, uint32_t n, int64_t now, const uint32_t* key_peer,
                                  uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids, const wgcs_keypairs* kp,
                                  uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(rekey_recv_gate_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, pkts, n, now, key_peer,
                     n_keys, peer_rows, n_ids, kp, n_peers);
  return hipGetLastError();
}

hipError_t launch_rekey_send_gate(const uint32_t* peer, const int32_t* count, const int32_t* status_in, uint32_t n_jobs,
                                  uint32_t max_segs, int64_t now, const uint32_t* peer_rows, uint32_t n_ids,
                                  const wgcs_keypairs* kp, uint32_t n_peers, const uint64_t* send_nonce,
                                  uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey, int32_t* status_out,
                                  hipStream_t s) {
  hipLaunchKernelGGL(rekey_send_gate_kernel, dim3(compact_blocks(n_jobs)), dim3(kThreads), 0, s, peer, count, status_in,
                     n_jobs, max_segs, now, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, limit, rekey,
                     status_out);
  return hipGetLastError();
}

hipError_t launch_rekey_sent(const uint32_t* peer, const int32_t* count, const int32_t* status, const uint32_t* job_key,
                             uint32_t n_jobs, uint32_t max_segs, int64_t now, const uint32_t* peer_rows,
                             uint32_t n_ids, const wgcs_keypairs* kp, uint32_t n_peers, const uint64_t* send_nonce,
                             uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey, hipStream_t s) {
  hipLaunchKernelGGL(rekey_sent_kernel, dim3(compact_blocks(n_jobs)), dim3(kThreads), 0, s, peer, count, status,
                     job_key, n_jobs, max_segs, now, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, limit, rekey);
  return hipGetLastError();
}

hipError_t launch_rekey_received(const wgcs_write_group* groups, uint32_t n, int64_t now, const uint32_t* peer_rows,
                                 uint32_t n_ids, const wgcs_keypairs* kp, uint32_t n_peers, wgcs_rekey* rekey,
                                 hipStream_t s) {
  hipLaunchKernelGGL(rekey_received_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, groups, n, now, peer_rows,
                     n_ids, kp, n_peers, rekey);
  return hipGetLastError();
}

hipError_t launch_rekey_responded(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now,
                                  wgcs_rekey* rekey, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(rekey_responded_kernel, dim3(compact_blocks(n)), dim3(kThreads), 0, s, resp, gate, n, now, rekey,
                     n_peers);
  return hipGetLastError();
}

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
