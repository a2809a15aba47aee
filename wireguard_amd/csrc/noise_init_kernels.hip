// noise_init_kernels.hip -- the initiator's half of the handshake on
// device-resident batches (include/wgcsum.h):
//   hs_initiate_kernel        CreateMessageInitiation and AddMACs      device/noise.go:344-403, cookie.go:287-314
//   hs_finish_kernel          ConsumeMessageResponse up to the state update, and the session keys
//                                                                      device/noise.go:548-604, :638-643
//   hs_finish_commit_kernel   the state update and the key rows of the responses that won
//                                                                      device/noise.go:606-620, :656-662
// One lane per row, as the kernels of noise_kernels.hip: a lane runs the row
// function of wgcs_noise.h, which the host forms of noise.cpp run too.  Both
// heavy kernels run two scalar multiplications in one ladder body; the commit
// kernel runs none.  A response may sit at any byte offset of the arena, which
// is read in aligned dwords and never written; every table row is 4-byte
// aligned.  Nothing draws randomness or reads a clock.
//
// Several responses of one batch may answer one handshake (a duplicated or
// replayed datagram).  hs_finish_kernel only reads the states, but for an
// atomicMin of the row number into the state's claim by every authentic row;
// hs_finish_commit_kernel, launched behind it on the same stream, lets the row
// that holds the claim commit and turns the others away, so the outcome does
// not depend on which wave ran first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_noise.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void hs_initiate_kernel(const wgcs_hs_start* __restrict__ start, uint32_t n,
                                                               const uint8_t* __restrict__ static_public,
                                                               const wgcs_peer_key* __restrict__ table,
                                                               uint32_t n_peers, uint32_t n_keys, wgcs_hs_state* states,
                                                               uint32_t n_states, uint8_t* msgs,
                                                               int32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  // the lane reads its own d_msgs row back for the two MACs
  status[q] = noise_initiate_row(start + q, static_public, table, n_peers, n_keys, states, n_states,
                                 msgs + kNoiseInitiationPitch * (uint64_t)q);
}

__global__ __launch_bounds__(kThreads) void hs_finish_kernel(const uint8_t* __restrict__ arena,
                                                             const wgcs_aead_pkt* __restrict__ pkts,
                                                             const int32_t* __restrict__ types,
                                                             const int32_t* __restrict__ gate, uint32_t n,
                                                             const wgcs_noise_responder* __restrict__ self,
                                                             const wgcs_session_slot* __restrict__ slots,
                                                             uint32_t n_slots, wgcs_hs_state* states, uint32_t n_states,
                                                             const uint8_t* __restrict__ psk, uint32_t n_peers,
                                                             uint32_t n_keys, uint8_t* __restrict__ work,
                                                             int32_t* __restrict__ verdict) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  verdict[q] =
      noise_finish_row(q, arena, pkts, types, gate, self, slots, n_slots, states, n_states, psk, n_peers, n_keys, work);
}

__global__ __launch_bounds__(kThreads) void hs_finish_commit_kernel(const uint8_t* __restrict__ arena,
                                                                    const wgcs_aead_pkt* __restrict__ pkts, uint32_t n,
                                                                    const wgcs_session_slot* __restrict__ slots,
                                                                    uint32_t n_slots, wgcs_hs_state* states,
                                                                    wgcs_aead_key* keys, uint8_t* __restrict__ work,
                                                                    int32_t* __restrict__ verdict) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  verdict[q] = noise_finish_commit(q, verdict[q], arena, pkts, slots, n_slots, states, keys, work);
}

}  // namespace

hipError_t launch_hs_initiate(const wgcs_hs_start* start, uint32_t n, const uint8_t* static_public,
                              const wgcs_peer_key* table, uint32_t n_peers, uint32_t n_keys, wgcs_hs_state* states,
                              uint32_t n_states, uint8_t* msgs, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(hs_initiate_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, start, n,
                     static_public, table, n_peers, n_keys, states, n_states, msgs, status);
  return hipGetLastError();
}

hipError_t launch_hs_finish(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types, const int32_t* gate,
                            uint32_t n, const wgcs_noise_responder* self, const wgcs_session_slot* slots,
                            uint32_t n_slots, wgcs_hs_state* states, uint32_t n_states, const uint8_t* psk,
                            uint32_t n_peers, wgcs_aead_key* keys, uint32_t n_keys, uint8_t* work, int32_t* verdict,
                            hipStream_t s) {
  const dim3 grid((n + kThreads - 1) / kThreads), block(kThreads);
  hipLaunchKernelGGL(hs_finish_kernel, grid, block, 0, s, arena, pkts, types, gate, n, self, slots, n_slots, states,
                     n_states, psk, n_peers, n_keys, work, verdict);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hs_finish_commit_kernel, grid, block, 0, s, arena, pkts, n, slots, n_slots, states, keys, work,
                     verdict);
  return hipGetLastError();
}

}  // namespace wgcs
