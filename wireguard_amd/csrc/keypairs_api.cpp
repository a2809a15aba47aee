// keypairs_api.cpp -- C ABI of the device-resident keypair rotation (include/wgcsum.h):
//   wgcs_keypairs_begin_responder_batch   the tail of BeginSymmetricSession behind respond   device/noise.go:664-722
//   wgcs_keypairs_begin_initiator_batch   the same behind finish
//   wgcs_keypairs_received_batch          ReceivedWithNewKeypair                             :725-754, receive.go:418-429
// They run in keypairs_kernels.hip, the begin forms on the key order of
// keyorder.hip; every table and the workspace are the caller's device memory.
// The host functions of the same section are in keypairs.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"

using namespace wgcs;

namespace {

// what the two begin forms share: the tail of their argument lists
int check_begin_tail(wgcs_ctx* ctx, const int32_t* d_gate, uint32_t n, const wgcs_peer_key* d_table, uint32_t n_peers,
                     const wgcs_keypairs* d_kp, const wgcs_session_slot* d_slots, uint32_t n_slots,
                     const wgcs_session_slot* d_peer_keys, uint32_t n_peer_slots, const wgcs_aead_key* d_keys,
                     const uint32_t* d_key_peer, const int32_t* d_status, const void* d_work) {
  if (!d_gate || !d_status || !d_table || !d_kp || !d_keys || !d_key_peer || !d_work || (n_slots && !d_slots) ||
      (n_peer_slots && !d_peer_keys))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (d_gate == d_status) return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_status must not be d_gate");
  if (n > kKeyOrderMaxRows || n_peers > kKeyOrderMaxKeys || !pow2_or_0(n_slots) || !pow2_or_0(n_peer_slots))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n, n_peers <= 2^24, n_slots and n_peer_slots 0 or a power of two");
  if (misaligned(d_gate, 3) || misaligned(d_status, 3) || misaligned(d_table, 3) || misaligned(d_kp, 3) ||
      misaligned(d_slots, 3) || misaligned(d_peer_keys, 3) || misaligned(d_keys, 3) || misaligned(d_key_peer, 3) ||
      misaligned(d_work, 15))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned tables, 16-byte aligned d_work");
  return WGCS_OK;
}

}  // namespace

extern "C" {

int wgcs_keypairs_begin_responder_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, const int32_t* d_gate, uint32_t n,
                                        int64_t now_ns, const wgcs_peer_key* d_table, uint32_t n_peers,
                                        wgcs_keypairs* d_kp, wgcs_session_slot* d_slots, uint32_t n_slots,
                                        wgcs_session_slot* d_peer_keys, uint32_t n_peer_slots, wgcs_aead_key* d_keys,
                                        uint32_t* d_key_peer, uint32_t n_keys, int32_t* d_status, void* d_work,
                                        size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_resp) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (int rc = check_begin_tail(ctx, d_gate, n, d_table, n_peers, d_kp, d_slots, n_slots, d_peer_keys, n_peer_slots,
                                d_keys, d_key_peer, d_status, d_work))
    return rc;
  if (misaligned(d_resp, 3)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned d_resp");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KeyOrder ko;
  if (int rc = keyorder_prepare(ctx, d_work, work_bytes, n, n_peers, s, &ko)) return rc;
  const hipError_t e = launch_keypairs_begin_responder(ko, d_resp, d_gate, n, now_ns, d_table, n_peers, d_kp, d_slots,
                                                       n_slots, d_peer_keys, n_peer_slots, d_keys, d_key_peer, n_keys,
                                                       d_status, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "keypairs_begin_responder launch");
}

int wgcs_keypairs_begin_initiator_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts,
                                        const int32_t* d_gate, uint32_t n, int64_t now_ns,
                                        const wgcs_session_slot* d_hs_slots, uint32_t n_hs_slots,
                                        const wgcs_hs_state* d_states, uint32_t n_states, const wgcs_peer_key* d_table,
                                        uint32_t n_peers, wgcs_keypairs* d_kp, wgcs_session_slot* d_slots,
                                        uint32_t n_slots, wgcs_session_slot* d_peer_keys, uint32_t n_peer_slots,
                                        wgcs_aead_key* d_keys, uint32_t* d_key_peer, uint32_t n_keys, int32_t* d_status,
                                        void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || (n_hs_slots && !d_hs_slots) || (n_states && !d_states))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (int rc = check_begin_tail(ctx, d_gate, n, d_table, n_peers, d_kp, d_slots, n_slots, d_peer_keys, n_peer_slots,
                                d_keys, d_key_peer, d_status, d_work))
    return rc;
  if (!pow2_or_0(n_hs_slots) || misaligned(d_pkts, 7) || misaligned(d_hs_slots, 3) || misaligned(d_states, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n_hs_slots 0 or a power of two, 8-byte aligned d_pkts, 4-byte aligned d_hs_slots / d_states");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KeyOrder ko;
  if (int rc = keyorder_prepare(ctx, d_work, work_bytes, n, n_peers, s, &ko)) return rc;
  const hipError_t e = launch_keypairs_begin_initiator(ko, d_arena, d_pkts, d_gate, n, now_ns, d_hs_slots, n_hs_slots,
                                                       d_states, n_states, d_table, n_peers, d_kp, d_slots, n_slots,
                                                       d_peer_keys, n_peer_slots, d_keys, d_key_peer, n_keys, d_status,
                                                       s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "keypairs_begin_initiator launch");
}

int wgcs_keypairs_received_batch(wgcs_ctx* ctx, const wgcs_aead_pkt* d_pkts, const int32_t* d_verdict, uint32_t n,
                                 uint32_t* d_key_peer, uint32_t n_keys, const uint32_t* d_peer_rows, uint32_t n_ids,
                                 wgcs_keypairs* d_kp, uint32_t n_peers, wgcs_session_slot* d_slots, uint32_t n_slots,
                                 wgcs_session_slot* d_peer_keys, uint32_t n_peer_slots, wgcs_aead_key* d_keys,
                                 uint32_t* d_rotated, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_pkts || !d_verdict || !d_rotated || (n_keys && (!d_key_peer || !d_keys)) || (n_ids && !d_peer_rows) ||
      (n_peers && !d_kp) || (n_slots && !d_slots) || (n_peer_slots && !d_peer_keys))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || !pow2_or_0(n_slots) || !pow2_or_0(n_peer_slots) || misaligned(d_pkts, 7) ||
      misaligned(d_verdict, 3) || misaligned(d_rotated, 3) || misaligned(d_key_peer, 3) || misaligned(d_keys, 3) ||
      misaligned(d_peer_rows, 3) || misaligned(d_kp, 3) || misaligned(d_slots, 3) || misaligned(d_peer_keys, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, n_slots and n_peer_slots 0 or a power of two, 8-byte aligned d_pkts, 4-byte aligned "
                   "tables");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_keypairs_received(d_pkts, d_verdict, n, d_key_peer, n_keys, d_peer_rows, n_ids, d_kp,
                                                n_peers, d_slots, n_slots, d_peer_keys, n_peer_slots, d_keys, d_rotated,
                                                stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "keypairs_received launch");
}

}  // extern "C"
