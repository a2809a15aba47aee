// keypairs_kernels.hip -- keypair rotation on device-resident tables
// (include/wgcsum.h), the row functions of wgcs_keypairs.h one lane at a time:
//   begin      the tail of BeginSymmetricSession          device/noise.go:664-722, sessions.go:70-82
//     kp_begin_resp_keys_kernel / kp_begin_init_keys_kernel   the gate and the stateless checks of every
//                                descriptor, and its peer row as the key of the key order
//     kp_begin_resp_groups_kernel / kp_begin_init_groups_kernel   the lane walk of wgcs_keyorder.h:
//                                one lane per peer takes that peer's descriptors in descriptor order
//   received   ReceivedWithNewKeypair                     noise.go:725-754, receive.go:418-429
//     kp_received_claim_kernel   the candidates, and the lowest of each peer by atomicMin
//     kp_received_commit_kernel  the rotation by the rows that hold their claim
// A rotation is sequential per peer and touches only that peer's row of d_kp,
// the slots of its own indices and its own key rows, so peers run side by
// side; the slot arrays keep their occupied slots, so a probe never breaks.
// Begin is rare and small (a handshake per peer every two minutes); the claim
// kernel is the one on the per-packet path: a row that is no candidate costs
// three dependent loads (key -> peer id -> peer row -> next) and one store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_keypairs.h"

namespace wgcs {

namespace {

constexpr int kThreads = kKeyOrderThreads;

// the stateless checks of keypairs_begin, so that a descriptor that fails them joins no peer's run
__device__ inline bool begin_fields_ok(const uint32_t f[4], uint32_t n_peers, uint32_t n_keys) {
  return f[0] < n_peers && f[2] < n_keys && f[3] < n_keys && f[2] != f[3];
}

__global__ __launch_bounds__(kThreads) void kp_begin_resp_keys_kernel(const wgcs_hs_resp* __restrict__ resp,
                                                                      const int32_t* __restrict__ gate, uint32_t n,
                                                                      uint32_t n_peers, uint32_t n_keys,
                                                                      int32_t* __restrict__ status,
                                                                      uint32_t* __restrict__ keys_in,
                                                                      uint32_t* __restrict__ slots_in) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  uint32_t f[4], key = n_peers;
  int st = WGCS_HS_NONE;
  if (keypairs_responder_fields(resp, gate, j, f)) {
    st = WGCS_ERR_INVALID_ARG;
    if (begin_fields_ok(f, n_peers, n_keys)) key = f[0];  // the peer's lane writes the status
  }
  if (key == n_peers) status[j] = st;
  keyorder_put(keys_in, slots_in, j, key);
}

__global__ __launch_bounds__(kThreads) void kp_begin_init_keys_kernel(
    const uint8_t* __restrict__ arena, const wgcs_aead_pkt* __restrict__ pkts, const int32_t* __restrict__ gate,
    uint32_t n, const wgcs_session_slot* __restrict__ hs_slots, uint32_t n_hs_slots,
    const wgcs_hs_state* __restrict__ states, uint32_t n_states, uint32_t n_peers, uint32_t n_keys,
    int32_t* __restrict__ status, uint32_t* __restrict__ keys_in, uint32_t* __restrict__ slots_in) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  uint32_t f[4], key = n_peers;
  int st = keypairs_initiator_fields(arena, pkts, gate, q, hs_slots, n_hs_slots, states, n_states, f);
  if (st == kKeypairsTaken) {
    st = WGCS_ERR_INVALID_ARG;
    if (begin_fields_ok(f, n_peers, n_keys)) key = f[0];
  }
  if (key == n_peers) status[q] = st;
  keyorder_put(keys_in, slots_in, q, key);
}

// Lane h owns the run of the key order that starts at heads[h]: one peer's descriptors, lowest first.
__global__ __launch_bounds__(kThreads) void kp_begin_resp_groups_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ heads,
    const uint32_t* __restrict__ n_heads, uint32_t n, const wgcs_hs_resp* __restrict__ resp,
    const int32_t* __restrict__ gate, int64_t now, const wgcs_peer_key* __restrict__ table, uint32_t n_peers,
    wgcs_keypairs* kp, wgcs_session_slot* d_slots, uint32_t n_slots, wgcs_session_slot* peer_keys,
    uint32_t n_peer_slots, wgcs_aead_key* aead_keys, uint32_t* key_peer, uint32_t n_keys, int32_t* status) {
  for (KeyRun r(keys, heads, n_heads, n, blockIdx.x * kThreads + threadIdx.x); r.more(); ++r.p) {
    const uint32_t j = slots[r.p];
    uint32_t f[4];
    keypairs_responder_fields(resp, gate, j, f);  // taken: the keys kernel saw it so
    status[j] = keypairs_begin(f[0], f[1], f[2], f[3], false, now, table, n_peers, kp, d_slots, n_slots, peer_keys,
                               n_peer_slots, aead_keys, key_peer, n_keys);
  }
}

__global__ __launch_bounds__(kThreads) void kp_begin_init_groups_kernel(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ heads,
    const uint32_t* __restrict__ n_heads, uint32_t n, const uint8_t* __restrict__ arena,
    const wgcs_aead_pkt* __restrict__ pkts, const int32_t* __restrict__ gate, int64_t now,
    const wgcs_session_slot* __restrict__ hs_slots, uint32_t n_hs_slots, const wgcs_hs_state* __restrict__ states,
    uint32_t n_states, const wgcs_peer_key* __restrict__ table, uint32_t n_peers, wgcs_keypairs* kp,
    wgcs_session_slot* d_slots, uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
    wgcs_aead_key* aead_keys, uint32_t* key_peer, uint32_t n_keys, int32_t* status) {
  for (KeyRun r(keys, heads, n_heads, n, blockIdx.x * kThreads + threadIdx.x); r.more(); ++r.p) {
    const uint32_t q = slots[r.p];
    uint32_t f[4];
    // the states are only read: the row answers as it did to the keys kernel
    const int rc = keypairs_initiator_fields(arena, pkts, gate, q, hs_slots, n_hs_slots, states, n_states, f);
    status[q] = rc != kKeypairsTaken ? rc
                              : keypairs_begin(f[0], f[1], f[2], f[3], true, now, table, n_peers, kp, d_slots, n_slots,
                                               peer_keys, n_peer_slots, aead_keys, key_peer, n_keys);
  }
}

__global__ __launch_bounds__(kThreads) void kp_received_claim_kernel(
    const wgcs_aead_pkt* __restrict__ pkts, const int32_t* __restrict__ verdict, uint32_t n,
    const uint32_t* __restrict__ key_peer, uint32_t n_keys, const uint32_t* __restrict__ peer_rows, uint32_t n_ids,
    wgcs_keypairs* kp, uint32_t n_peers, uint32_t* __restrict__ rotated) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  rotated[i] = keypairs_received_claim(i, pkts, verdict, key_peer, n_keys, peer_rows, n_ids, kp, n_peers);
}

__global__ __launch_bounds__(kThreads) void kp_received_commit_kernel(
    const wgcs_aead_pkt* __restrict__ pkts, uint32_t n, uint32_t* key_peer, uint32_t n_keys,
    const uint32_t* __restrict__ peer_rows, uint32_t n_ids, wgcs_keypairs* kp, uint32_t n_peers,
    wgcs_session_slot* d_slots, uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
    wgcs_aead_key* aead_keys, uint32_t* __restrict__ rotated) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n || rotated[i] == 0) return;  // only a candidate looks its peer up again
  rotated[i] = keypairs_received_commit(i, pkts, key_peer, n_keys, peer_rows, n_ids, kp, n_peers, d_slots, n_slots,
                                        peer_keys, n_peer_slots, aead_keys);
}

}  // namespace

hipError_t launch_keypairs_begin_responder(const KeyOrder& ko, const wgcs_hs_resp* resp, const int32_t* gate,
                                           uint32_t n, int64_t now, const wgcs_peer_key* table, uint32_t n_peers,
                                           wgcs_keypairs* kp, wgcs_session_slot* slots, uint32_t n_slots,
                                           wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys,
                                           uint32_t* key_peer, uint32_t n_keys, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(kp_begin_resp_keys_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, resp, gate, n, n_peers,
                     n_keys, status, ko.keys_in, ko.slots_in);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = keyorder_sort(ko, n, n_peers, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(kp_begin_resp_groups_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, ko.keys, ko.slots,
                     ko.heads, ko.n_heads, n, resp, gate, now, table, n_peers, kp, slots, n_slots, peer_keys,
                     n_peer_slots, keys, key_peer, n_keys, status);
  return hipGetLastError();
}

hipError_t launch_keypairs_begin_initiator(const KeyOrder& ko, const uint8_t* arena, const wgcs_aead_pkt* pkts,
                                           const int32_t* gate, uint32_t n, int64_t now,
                                           const wgcs_session_slot* hs_slots, uint32_t n_hs_slots,
                                           const wgcs_hs_state* states, uint32_t n_states, const wgcs_peer_key* table,
                                           uint32_t n_peers, wgcs_keypairs* kp, wgcs_session_slot* slots,
                                           uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                                           wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys, int32_t* status,
                                           hipStream_t s) {
  hipLaunchKernelGGL(kp_begin_init_keys_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, arena, pkts, gate, n,
                     hs_slots, n_hs_slots, states, n_states, n_peers, n_keys, status, ko.keys_in, ko.slots_in);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = keyorder_sort(ko, n, n_peers, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(kp_begin_init_groups_kernel, dim3(keyorder_blocks(n)), dim3(kThreads), 0, s, ko.keys, ko.slots,
                     ko.heads, ko.n_heads, n, arena, pkts, gate, now, hs_slots, n_hs_slots, states, n_states, table,
                     n_peers, kp, slots, n_slots, peer_keys, n_peer_slots, keys, key_peer, n_keys, status);
  return hipGetLastError();
}

hipError_t launch_keypairs_received(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n, uint32_t* key_peer,
                                    uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids, wgcs_keypairs* kp,
                                    uint32_t n_peers, wgcs_session_slot* slots, uint32_t n_slots,
                                    wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys,
                                    uint32_t* rotated, hipStream_t s) {
  const dim3 grid(keyorder_blocks(n)), block(kThreads);
  hipLaunchKernelGGL(kp_received_claim_kernel, grid, block, 0, s, pkts, verdict, n, key_peer, n_keys, peer_rows, n_ids,
                     kp, n_peers, rotated);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kp_received_commit_kernel, grid, block, 0, s, pkts, n, key_peer, n_keys, peer_rows, n_ids, kp,
                     n_peers, slots, n_slots, peer_keys, n_peer_slots, keys, rotated);
  return hipGetLastError();
}

}  // namespace wgcs
