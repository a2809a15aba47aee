// rekey_kernels.hip -- keypair expiry, the rekey rules and the start of a
// handshake on device-resident tables (include/wgcsum.h), the row functions of
// wgcs_rekey.h one lane at a time:
//   rekey_recv_gate_kernel     a packet under a keypair past RejectAfterTime      receive.go:162-170
//   rekey_send_gate_kernel     a job without a usable current keypair             send.go:368-374
//   rekey_sent_kernel          keepKeyFreshSending behind send-assign             send.go:213-227, :419-420
//   rekey_received_kernel      keepKeyFreshReceiving over the write groups        receive.go:80-91
//   rekey_responded_kernel     lastSentHandshake behind respond                   send.go:131-133
//   start                      SendHandshakeInitiation over the peer rows         send.go:84-100
//     rekey_start_verdict_kernel   the wish and the timeout of every row, the candidates of each block counted
//     rekey_start_scan_kernel      the block counts into the candidates in front of each block, and *d_count
//     rekey_start_commit_kernel    the descriptor of every candidate that has a ticket, and the tail rows
// The gates are on the per-packet path: a row costs three dependent loads
// (key or peer id -> peer row -> keypair) and, when its keypair is stale, one
// store.  Rows of one peer only OR bits into its wgcs_rekey row or store the
// call's clock there, so the tables do not depend on which wave ran first; the
// rank of a start candidate -- the candidates in the rows below it -- is a sum
// of whole-block counts and of a ballot inside its block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_rekey.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;  // gfx950 runs these kernels in wave64
constexpr int kScanThreads = 1024;

inline uint32_t blocks_for(uint32_t n) { return n / kThreads + (n % kThreads != 0); }

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
  const int cand = __syncthreads_count(r < n_peers && v == WGCS_HS_STARTED);
  if (threadIdx.x == 0) block_cand[blockIdx.x] = (uint32_t)cand;
}

// One block: block_cand[b] becomes the candidates of the blocks below b, 1,024 blocks a turn,
// and *count the descriptors the commit kernel writes.
__global__ __launch_bounds__(kScanThreads) void rekey_start_scan_kernel(uint32_t* __restrict__ block_cand,
                                                                        uint32_t n_blocks, uint32_t n_tickets,
                                                                        uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_sum[kScanThreads / kWave];
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  uint32_t below = 0;  // the candidates of every block of the turns before this one
  for (uint32_t first = 0; first < n_blocks; first += kScanThreads) {
    const uint32_t b = first + threadIdx.x;
    const uint32_t mine = b < n_blocks ? block_cand[b] : 0;
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
    if (b < n_blocks) block_cand[b] = below + waves_below + x - mine;
    below += turn;
    __syncthreads();  // wave_sum is written again in the next turn
  }
  if (threadIdx.x == 0) *count = below < n_tickets ? below : n_tickets;
}

// The grid covers max(n_peers, n_tickets) rows: lane q commits peer row q if it is a candidate,
// and fills descriptor q if it lies past the count.  A candidate's descriptor lies below the
// count, so no two lanes write one descriptor.
__global__ __launch_bounds__(kThreads) void rekey_start_commit_kernel(
    int64_t now, wgcs_rekey* rekey, const wgcs_hs_peer* __restrict__ hs_peers, uint32_t n_peers,
    const wgcs_hs_start* __restrict__ tickets, uint32_t n_tickets, wgcs_hs_start* __restrict__ start,
    uint32_t* __restrict__ start_peer, const uint32_t* __restrict__ count, const uint32_t* __restrict__ cand_below,
    int32_t* __restrict__ status) {
  __shared__ uint32_t wave_cand[kThreads / kWave];
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const bool cand = q < n_peers && status[q] == WGCS_HS_STARTED;
  const uint64_t ballot = __ballot(cand);
  if (lane == 0) wave_cand[wave] = (uint32_t)__popcll(ballot);
  __syncthreads();
  if (cand) {  // a block with a candidate is a block of the verdict kernel's grid: cand_below has its word
    uint32_t rank = cand_below[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1));
    for (uint32_t w = 0; w < wave; ++w) rank += wave_cand[w];
    status[q] = rekey_start_commit(q, rank, now, rekey, hs_peers, tickets, n_tickets, start, start_peer);
  }
  if (q < n_tickets && q >= *count) rekey_start_tail(q, start, start_peer);
}

}  // namespace

hipError_t launch_rekey_recv_gate(wgcs_aead_pkt* pkts, uint32_t n, int64_t now, const uint32_t* key_peer,
                                  uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids, const wgcs_keypairs* kp,
                                  uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(rekey_recv_gate_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, pkts, n, now, key_peer, n_keys,
                     peer_rows, n_ids, kp, n_peers);
  return hipGetLastError();
}

hipError_t launch_rekey_send_gate(const uint32_t* peer, const int32_t* count, const int32_t* status_in, uint32_t n_jobs,
                                  uint32_t max_segs, int64_t now, const uint32_t* peer_rows, uint32_t n_ids,
                                  const wgcs_keypairs* kp, uint32_t n_peers, const uint64_t* send_nonce,
                                  uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey, int32_t* status_out,
                                  hipStream_t s) {
  hipLaunchKernelGGL(rekey_send_gate_kernel, dim3(blocks_for(n_jobs)), dim3(kThreads), 0, s, peer, count, status_in,
                     n_jobs, max_segs, now, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, limit, rekey,
                     status_out);
  return hipGetLastError();
}

hipError_t launch_rekey_sent(const uint32_t* peer, const int32_t* count, const int32_t* status, const uint32_t* job_key,
                             uint32_t n_jobs, uint32_t max_segs, int64_t now, const uint32_t* peer_rows,
                             uint32_t n_ids, const wgcs_keypairs* kp, uint32_t n_peers, const uint64_t* send_nonce,
                             uint32_t n_keys, uint64_t limit, wgcs_rekey* rekey, hipStream_t s) {
  hipLaunchKernelGGL(rekey_sent_kernel, dim3(blocks_for(n_jobs)), dim3(kThreads), 0, s, peer, count, status, job_key,
                     n_jobs, max_segs, now, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, limit, rekey);
  return hipGetLastError();
}

hipError_t launch_rekey_received(const wgcs_write_group* groups, uint32_t n, int64_t now, const uint32_t* peer_rows,
                                 uint32_t n_ids, const wgcs_keypairs* kp, uint32_t n_peers, wgcs_rekey* rekey,
                                 hipStream_t s) {
  hipLaunchKernelGGL(rekey_received_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, groups, n, now, peer_rows,
                     n_ids, kp, n_peers, rekey);
  return hipGetLastError();
}

hipError_t launch_rekey_responded(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now,
                                  wgcs_rekey* rekey, uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(rekey_responded_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, resp, gate, n, now, rekey,
                     n_peers);
  return hipGetLastError();
}

hipError_t launch_rekey_start(int64_t now, wgcs_rekey* rekey, const wgcs_hs_peer* hs_peers, uint32_t n_peers,
                              const wgcs_hs_start* tickets, uint32_t n_tickets, wgcs_hs_start* start,
                              uint32_t* start_peer, uint32_t* count, int32_t* status, uint32_t* reasons,
                              uint32_t* block_cand, hipStream_t s) {
  const uint32_t n_blocks = blocks_for(n_peers);
  hipError_t e;
  if (n_blocks) {
    hipLaunchKernelGGL(rekey_start_verdict_kernel, dim3(n_blocks), dim3(kThreads), 0, s, now, rekey, n_peers, status,
                       reasons, block_cand);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rekey_start_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, block_cand, n_blocks, n_tickets,
                     count);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t rows = n_peers > n_tickets ? n_peers : n_tickets;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(rekey_start_commit_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, s, now, rekey, hs_peers,
                     n_peers, tickets, n_tickets, start, start_peer, count, block_cand, status);
  return hipGetLastError();
}

}  // namespace wgcs
