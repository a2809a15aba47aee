// noise_api.cpp -- C ABI of the device-resident X25519 and handshake consume (include/wgcsum.h):
//   wgcs_x25519_batch               curve25519.X25519, one per row     device/noise_helpers.go:93-105
//   wgcs_handshake_consume_batch    ConsumeMessageInitiation to :457   device/noise.go:405-457
//   wgcs_handshake_respond_batch    CreateMessageResponse, AddMACs, the responder's keys   :494-546, :646-651
//   wgcs_handshake_initiate_batch   CreateMessageInitiation, AddMACs, the handshake state  :344-403
//   wgcs_handshake_finish_batch     ConsumeMessageResponse, the initiator's keys           :548-620, :636-662
//   wgcs_handshake_accept_batch     the timestamp and flood rules, the responder's state     :458-491
// They run in noise_kernels.hip, noise_init_kernels.hip and noise_accept_kernels.hip; the responder, the
// tables and the rows are the caller's device memory.  The host functions of
// the same sections are in noise.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_compact.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"

using namespace wgcs;

extern "C" {

int wgcs_x25519_batch(wgcs_ctx* ctx, const uint8_t* d_scalars, const uint8_t* d_points, uint32_t n, uint8_t* d_out,
                      int32_t* d_status, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_scalars || !d_points || !d_out || !d_status) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_scalars & 3) || ((uintptr_t)d_points & 3) || ((uintptr_t)d_out & 3) ||
      ((uintptr_t)d_status & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 4-byte aligned d_scalars / d_points / d_out / d_status");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e =
      launch_x25519(d_scalars, d_points, n, d_out, d_status, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "x25519 launch");
}

int wgcs_handshake_consume_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts,
                                 const int32_t* d_type, const int32_t* d_gate, uint32_t n,
                                 const wgcs_noise_responder* d_responder, const wgcs_peer_key* d_table,
                                 uint32_t n_peers, int32_t* d_verdict, wgcs_hs_init* d_out, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_type || !d_responder || !d_verdict || !d_out || (n_peers && !d_table))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (d_gate == d_verdict) return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_verdict must not be d_gate");
  if (n > kMaxRows || ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_type & 3) || ((uintptr_t)d_gate & 3) ||
      ((uintptr_t)d_responder & 3) || ((uintptr_t)d_table & 3) || ((uintptr_t)d_verdict & 3) || ((uintptr_t)d_out & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, 8-byte aligned d_pkts, 4-byte aligned d_type / d_gate / d_responder / d_table / "
                   "d_verdict / d_out");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_hs_consume(d_arena, d_pkts, d_type, d_gate, n, d_responder, d_table, n_peers, d_verdict,
                                         d_out, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "handshake_consume launch");
}

int wgcs_handshake_respond_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, uint32_t n, const wgcs_hs_init* d_init,
                                 const int32_t* d_gate, uint32_t n_init, const wgcs_peer_key* d_table,
                                 const uint8_t* d_psk, uint32_t n_peers, wgcs_aead_key* d_keys, uint32_t n_keys,
                                 uint8_t* d_msgs, int32_t* d_status, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_resp || !d_msgs || !d_status || (n_init && !d_init) || (n_peers && !d_table) || (n_keys && !d_keys))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_resp & 3) || ((uintptr_t)d_init & 3) || ((uintptr_t)d_gate & 3) ||
      ((uintptr_t)d_table & 3) || ((uintptr_t)d_psk & 3) || ((uintptr_t)d_keys & 3) || ((uintptr_t)d_msgs & 3) ||
      ((uintptr_t)d_status & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, 4-byte aligned d_resp / d_init / d_gate / d_table / d_psk / d_keys / d_msgs / d_status");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_hs_respond(d_resp, n, d_init, d_gate, n_init, d_table, d_psk, n_peers, d_keys, n_keys,
                                         d_msgs, d_status, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "handshake_respond launch");
}

int wgcs_handshake_initiate_batch(wgcs_ctx* ctx, const wgcs_hs_start* d_start, uint32_t n,
                                  const uint8_t* d_static_public, const wgcs_peer_key* d_table, uint32_t n_peers,
                                  uint32_t n_keys, wgcs_hs_state* d_states, uint32_t n_states, uint8_t* d_msgs,
                                  int32_t* d_status, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_start || !d_static_public || !d_msgs || !d_status || (n_peers && !d_table) || (n_states && !d_states))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_start & 3) || ((uintptr_t)d_static_public & 3) || ((uintptr_t)d_table & 3) ||
      ((uintptr_t)d_states & 3) || ((uintptr_t)d_msgs & 3) || ((uintptr_t)d_status & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, 4-byte aligned d_start / d_static_public / d_table / d_states / d_msgs / d_status");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_hs_initiate(d_start, n, d_static_public, d_table, n_peers, n_keys, d_states, n_states,
                                          d_msgs, d_status, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "handshake_initiate launch");
}

int wgcs_handshake_finish_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts,
                                const int32_t* d_type, const int32_t* d_gate, uint32_t n,
                                const wgcs_noise_responder* d_responder, const wgcs_session_slot* d_slots,
                                uint32_t n_slots, wgcs_hs_state* d_states, uint32_t n_states, const uint8_t* d_psk,
                                uint32_t n_peers, wgcs_aead_key* d_keys, uint32_t n_keys, uint8_t* d_work,
                                int32_t* d_verdict, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_type || !d_responder || !d_work || !d_verdict || (n_slots && !d_slots) ||
      (n_states && !d_states) || (n_keys && !d_keys))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (d_gate == d_verdict) return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_verdict must not be d_gate");
  if (n > kMaxRows || (n_slots & (n_slots - 1)) || ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_type & 3) ||
      ((uintptr_t)d_gate & 3) || ((uintptr_t)d_responder & 3) || ((uintptr_t)d_slots & 3) ||
      ((uintptr_t)d_states & 3) || ((uintptr_t)d_psk & 3) || ((uintptr_t)d_keys & 3) || ((uintptr_t)d_work & 3) ||
      ((uintptr_t)d_verdict & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, n_slots 0 or a power of two, 8-byte aligned d_pkts, 4-byte aligned d_type / d_gate / "
                   "d_responder / d_slots / d_states / d_psk / d_keys / d_work / d_verdict");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e =
      launch_hs_finish(d_arena, d_pkts, d_type, d_gate, n, d_responder, d_slots, n_slots, d_states, n_states, d_psk,
                       n_peers, d_keys, n_keys, d_work, d_verdict, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "handshake_finish launch");
}

int wgcs_handshake_accept_batch(wgcs_ctx* ctx, const wgcs_hs_init* d_init, const int32_t* d_gate, uint32_t n,
                                int64_t now_ns, const wgcs_peer_key* d_table, const uint32_t* d_peer_rows,
                                uint32_t n_ids, wgcs_hs_peer* d_peers, uint32_t n_peers,
                                const wgcs_hs_ticket* d_tickets, uint32_t n_tickets, wgcs_hs_resp* d_resp,
                                uint32_t* d_count, int32_t* d_verdict, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!d_count || (n && (!d_init || !d_gate || !d_verdict)) || (n_tickets && (!d_tickets || !d_resp)) ||
      (n && n_peers && (!d_table || !d_peers)) || (n && n_ids && !d_peer_rows))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n && (const int32_t*)d_verdict == d_gate) return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_verdict must not be d_gate");
  if (n > kMaxRows || n_tickets > kMaxRows || ((uintptr_t)d_init & 3) || ((uintptr_t)d_gate & 3) ||
      ((uintptr_t)d_table & 3) || ((uintptr_t)d_peer_rows & 3) || ((uintptr_t)d_peers & 3) ||
      ((uintptr_t)d_tickets & 3) || ((uintptr_t)d_resp & 3) || ((uintptr_t)d_count & 3) || ((uintptr_t)d_verdict & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n and n_tickets <= 2^28, 4-byte aligned d_init / d_gate / d_table / d_peer_rows / d_peers / "
                   "d_tickets / d_resp / d_count / d_verdict");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  hipError_t e;
  // the block counts are the context's: the call before this one, if another stream holds it, is done with them first
  if (ctx->accept_pending && ctx->accept_stream != s &&
      (e = hipStreamWaitEvent(s, ctx->accept_ev, 0)) != hipSuccess)
    return hip_fail(ctx, e, "handshake_accept stream order");
  const int rc = ensure_dev(ctx, ctx->d_accept, sizeof(uint32_t) * (size_t)(compact_blocks(n) + 1));
  if (rc != WGCS_OK) return rc;
  e = launch_hs_accept(d_init, d_gate, n, now_ns, d_table, d_peer_rows, n_ids, d_peers, n_peers, d_tickets, n_tickets,
                       d_resp, d_count, d_verdict, (uint32_t*)ctx->d_accept.ptr, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "handshake_accept launch");
  if ((e = hipEventRecord(ctx->accept_ev, s)) != hipSuccess) return hip_fail(ctx, e, "handshake_accept event");
  ctx->accept_stream = s;
  ctx->accept_pending = true;
  return WGCS_OK;
}

}  // extern "C"
