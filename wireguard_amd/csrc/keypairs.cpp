// keypairs.cpp -- keypair rotation on host memory (include/wgcsum.h), no context
// and no device:
//   wgcs_keypairs_begin_responder_host   the tail of BeginSymmetricSession behind respond   device/noise.go:664-722
//   wgcs_keypairs_begin_initiator_host   the same behind finish
//   wgcs_keypairs_received_host          ReceivedWithNewKeypair, in its two passes          :725-754, receive.go:418-429
// They run the row functions of wgcs_keypairs.h, the code the lanes of
// keypairs_kernels.hip run, taken in row order.  Plain C++: the host test
// program (tests/keypairs_host/keypairs_host.cpp) links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_keypairs.h"

using namespace wgcs;

namespace {

inline bool pow2_or_zero(uint32_t x) { return (x & (x - 1)) == 0; }

bool begin_args_ok(const void* rows, const int32_t* gate, uint32_t n, const wgcs_peer_key* table, uint32_t n_peers,
                   const wgcs_keypairs* kp, const wgcs_session_slot* slots, uint32_t n_slots,
                   const wgcs_session_slot* peer_keys, uint32_t n_peer_slots, const wgcs_aead_key* keys,
                   const uint32_t* key_peer, const int32_t* status) {
  return n <= kKeyOrderMaxRows && n_peers <= kMaxPeers && rows && gate && status && gate != status && table && kp && keys &&
         key_peer && pow2_or_zero(n_slots) && pow2_or_zero(n_peer_slots) && (!n_slots || slots) &&
         (!n_peer_slots || peer_keys);
}

}  // namespace

extern "C" {

int wgcs_keypairs_begin_responder_host(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now_ns,
                                       const wgcs_peer_key* table, uint32_t n_peers, wgcs_keypairs* kp,
                                       wgcs_session_slot* slots, uint32_t n_slots, wgcs_session_slot* peer_keys,
                                       uint32_t n_peer_slots, wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys,
                                       int32_t* status) {
  if (n == 0) return WGCS_OK;
  if (!begin_args_ok(resp, gate, n, table, n_peers, kp, slots, n_slots, peer_keys, n_peer_slots, keys, key_peer, status))
    return WGCS_ERR_INVALID_ARG;
  for (uint32_t j = 0; j < n; ++j) {
    uint32_t f[4];
    status[j] = !keypairs_responder_fields(resp, gate, j, f)
                    ? WGCS_HS_NONE
                    : keypairs_begin(f[0], f[1], f[2], f[3], false, now_ns, table, n_peers, kp, slots, n_slots,
                                     peer_keys, n_peer_slots, keys, key_peer, n_keys);
  }
  return WGCS_OK;
}

int wgcs_keypairs_begin_initiator_host(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* gate,
                                       uint32_t n, int64_t now_ns, const wgcs_session_slot* hs_slots,
                                       uint32_t n_hs_slots, const wgcs_hs_state* states, uint32_t n_states,
                                       const wgcs_peer_key* table, uint32_t n_peers, wgcs_keypairs* kp,
                                       wgcs_session_slot* slots, uint32_t n_slots, wgcs_session_slot* peer_keys,
                                       uint32_t n_peer_slots, wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys,
                                       int32_t* status) {
  if (n == 0) return WGCS_OK;
  if (!begin_args_ok(pkts, gate, n, table, n_peers, kp, slots, n_slots, peer_keys, n_peer_slots, keys, key_peer,
                     status) ||
      !arena || !pow2_or_zero(n_hs_slots) || (n_hs_slots && !hs_slots) || (n_states && !states))
    return WGCS_ERR_INVALID_ARG;
  for (uint32_t q = 0; q < n; ++q) {
    uint32_t f[4];
    const int rc = keypairs_initiator_fields(arena, pkts, gate, q, hs_slots, n_hs_slots, states, n_states, f);
    status[q] = rc != kKeypairsTaken ? rc
                              : keypairs_begin(f[0], f[1], f[2], f[3], true, now_ns, table, n_peers, kp, slots,
                                               n_slots, peer_keys, n_peer_slots, keys, key_peer, n_keys);
  }
  return WGCS_OK;
}

int wgcs_keypairs_received_host(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n, uint32_t* key_peer,
                                uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids, wgcs_keypairs* kp,
                                uint32_t n_peers, wgcs_session_slot* slots, uint32_t n_slots,
                                wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys,
                                uint32_t* rotated) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !pkts || !verdict || !rotated || (n_keys && (!key_peer || !keys)) || (n_ids && !peer_rows) ||
      (n_peers && !kp) || !pow2_or_zero(n_slots) || !pow2_or_zero(n_peer_slots) || (n_slots && !slots) ||
      (n_peer_slots && !peer_keys))
    return WGCS_ERR_INVALID_ARG;
  // the two launches of the device form, each a loop: every row sees the tables as they stood at the call
  for (uint32_t i = 0; i < n; ++i)
    rotated[i] = keypairs_received_claim(i, pkts, verdict, key_peer, n_keys, peer_rows, n_ids, kp, n_peers);
  for (uint32_t i = 0; i < n; ++i)
    if (rotated[i])
      rotated[i] = keypairs_received_commit(i, pkts, key_peer, n_keys, peer_rows, n_ids, kp, n_peers, slots, n_slots,
                                            peer_keys, n_peer_slots, keys);
  return WGCS_OK;
}

}  // extern "C"
